"""CPU test: csrc/plan_check.cpp, the stand-alone check of the launch plans
(pt_mk_plan.hpp, pt_wf_plan.hpp), builds with the Makefile's plan_check target
and passes. Host code only: no HIP runtime call, no GPU."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'path-tracer-python_amd', 'csrc')


def test_plan_check_passes(tmp_path):
    exe = str(tmp_path / 'plan_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'plan_check', f'PLAN_CHECK={exe}'], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert 'plans ok' in r.stdout
