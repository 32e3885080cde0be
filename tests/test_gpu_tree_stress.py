"""The rebuild parity and history cases of tests/test_gpu_tree.py with the
register-budget stress build (libptmi_stress.so, see
tests/test_gpu_stress_build.py): the rebuilt scene must render, and a history
must cross the rebuild, with the same bits when every render kernel spills.
Runs in a child process (the library is loaded once per process)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
STRESS = os.path.join(ROOT, 'path-tracer-python_amd', 'ptmi', '_lib', 'libptmi_stress.so')
CASES = ['test_rebuild_leaves_the_packed_compile_in_the_same_tensors[coverage]',
         'test_render_parity_after_the_rebuild_of_coverage',
         'test_render_parity_when_the_rebuild_changes_the_leaf_depth',
         'test_history_across_a_rebuild_equals_history_across_the_update']


def test_stress_build_tree():
    assert os.path.exists(STRESS), 'libptmi_stress.so missing: run __graft_entry__.build()'
    mod = os.path.join(ROOT, 'tests', 'test_gpu_tree.py')
    p = subprocess.run([sys.executable, '-m', 'pytest'] + [f'{mod}::{c}' for c in CASES] +
                       ['-q', '-x', '-p', 'no:cacheprovider'], env=dict(os.environ, PTMI_LIB=STRESS),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert f'{len(CASES)} passed' in p.stdout and 'skipped' not in p.stdout, p.stdout[-2000:]
