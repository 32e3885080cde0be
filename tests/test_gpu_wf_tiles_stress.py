"""The tile-listed wavefront GPU tests (tests/test_gpu_wf_tiles.py) with the
register-budget stress build (libptmi_stress.so, see
tests/test_gpu_stress_build.py): the listed trace, a short list with an odd
sample count and the adaptive loop must give the same bits when every render
kernel spills. Runs in a child process (the library is loaded once per
process)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
STRESS = os.path.join(ROOT, 'path-tracer-python_amd', 'ptmi', '_lib', 'libptmi_stress.so')
CASES = ['test_listed_trace_wf', 'test_short_lists[n7-s3-from0]', 'test_short_lists[n7-s3-from5]',
         'test_adaptive_end_to_end_wf']


def test_stress_build_wf_tiles():
    assert os.path.exists(STRESS), 'libptmi_stress.so missing: run __graft_entry__.build()'
    mod = os.path.join(ROOT, 'tests', 'test_gpu_wf_tiles.py')
    p = subprocess.run([sys.executable, '-m', 'pytest'] + [f'{mod}::{c}' for c in CASES] +
                       ['-q', '-x', '-p', 'no:cacheprovider'], env=dict(os.environ, PTMI_LIB=STRESS),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert f'{len(CASES)} passed' in p.stdout and 'skipped' not in p.stdout, p.stdout[-2000:]
