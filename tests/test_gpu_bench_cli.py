"""bench.py as a command on the GPU: a plain run (set up, warm up, time the
steps, --dump-outputs, the line) and a --full run (the per-kernel roofline and
the CPU baseline on top). Small calls: 2 steps of 2 spp."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
ARGS = ['--gpus', '1', '--spp-per-step', '2', '--steps', '2', '--warmup', '1']


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *ARGS, *extra], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_accumulator_it_timed(tmp_path):
    """The dump is the accumulator after the timed steps (--save-accum's array)
    and the same from run to run; the plain line has the headline figures and
    none of --full's."""
    rec = _bench('--dump-outputs', str(tmp_path / 'a'), '--save-accum', str(tmp_path / 'acc.npy'))
    a = np.load(tmp_path / 'a' / 'accum.npy')
    assert a.dtype == np.float32 and a.shape == (800, 800, 3) and a.sum() > 0
    assert np.array_equal(a, np.load(tmp_path / 'acc.npy'), equal_nan=True)
    assert rec['full'] is False and rec['steps'] == 2 and rec['warmup'] == 1
    assert rec['unit'] == 'Msamples/s' and rec['higher_is_better'] is True and rec['dtype'] == 'f32'
    assert rec['value'] > 0 and rec['ms_per_step'] > 0
    # value and ms_per_step are the same measurement: samples of a step / its time
    assert rec['value'] == pytest.approx(800 * 800 * 2 / rec['ms_per_step'] / 1e3, rel=1e-3)
    for k in ('roofline', 'kernels_ms', 'kernels_busy_ms', 'valu_diagnostic', 'cpu_baseline'):
        assert k not in rec
    _bench('--dump-outputs', str(tmp_path / 'b'))
    assert np.array_equal(a, np.load(tmp_path / 'b' / 'accum.npy'), equal_nan=True)


def test_full_run_adds_the_roofline_and_the_cpu_baseline():
    """--full on the wavefront: its kernels are timed in a second pass, the
    CPU oracle after it."""
    rec = _bench('--full', '--variant', 'wf', '--cpu-seconds', '0.2')
    assert rec['full'] is True and rec['value'] > 0 and rec['ms_per_step'] > 0
    assert rec['roofline']['kernel'] in rec['kernels_busy_ms'] and rec['roofline']['launches'] > 0
    assert 'second pass' in rec['roofline']['timing'] and rec['roofline']['achieved'] > 0
    assert rec['cpu_baseline']['value'] > 0 and rec['ranks'][0]['kernel_busy_ms'] > 0
