"""The scene-update GPU tests (tests/test_gpu_update.py) with the
register-budget stress build (libptmi_stress.so, see
tests/test_gpu_stress_build.py): the moved buffers and the renders after an
update must give the same bits when every render kernel spills. Runs in a child
process (the library is loaded once per process)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
STRESS = os.path.join(ROOT, 'path-tracer-python_amd', 'ptmi', '_lib', 'libptmi_stress.so')
CASES = ['test_moved_buffers_equal_the_packed_reference_and_the_inverse_restores_them[coverage-per_level]',
         'test_moved_buffers_equal_the_packed_reference_and_the_inverse_restores_them[vol2_final_scene-one_group]',
         'test_render_parity_after_the_update[coverage]', 'test_render_parity_after_the_update[vol2_final_scene]']


def test_stress_build_update():
    assert os.path.exists(STRESS), 'libptmi_stress.so missing: run __graft_entry__.build()'
    mod = os.path.join(ROOT, 'tests', 'test_gpu_update.py')
    p = subprocess.run([sys.executable, '-m', 'pytest'] + [f'{mod}::{c}' for c in CASES] +
                       ['-q', '-x', '-p', 'no:cacheprovider'], env=dict(os.environ, PTMI_LIB=STRESS),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert f'{len(CASES)} passed' in p.stdout and 'skipped' not in p.stdout, p.stdout[-2000:]
