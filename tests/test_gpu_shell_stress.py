"""The shell and pole cases of tests/test_gpu_shell.py with the register-budget
stress build (libptmi_stress.so, see tests/test_gpu_stress_build.py): the
SHELL kernels must give the same bits when they spill. Runs in a child process
(the library is loaded once per process)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
STRESS = os.path.join(ROOT, 'path-tracer-python_amd', 'ptmi', '_lib', 'libptmi_stress.so')


def test_stress_build_shell_cases():
    assert os.path.exists(STRESS), 'libptmi_stress.so missing: run __graft_entry__.build()'
    p = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_shell.py'), '-q', '-x',
                        '-p', 'no:cacheprovider', '-k', 'test_shell_scene or test_poles'],
                       env=dict(os.environ, PTMI_LIB=STRESS), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert '30 passed' in p.stdout and 'skipped' not in p.stdout, p.stdout[-2000:]
