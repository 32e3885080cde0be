"""CPU tests of the pose ABI's arithmetic (csrc/pt_pose_math.hpp, the functions
the kernel of csrc/pt_pose.hip calls), run by the stand-alone csrc/pose_check.cpp
against the Python definition (ptmi/pose.py): the row floats and the leaf boxes
equal ``scene_compiler.update_records`` of the posed objects and update_helpers'
box rules bit for bit, also under the sanitizers; t = 0 is not the rest row of a
quad with Q.x = -0.0; and the box at any t in (0, 1) lies within the union of
the boxes at 0 and 1, which is what DeviceScene.set_tracks' shell hint relies on."""
import os
import subprocess

import numpy as np
import pytest

import pose_helpers as psh
from ptmi import core, pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'path-tracer-python_amd', 'csrc')
f32 = np.float32
MODE = {'spheres': 'sphere', 'quads': 'quad', 'triangles': 'tri'}
N_TRACKS = 200


@pytest.fixture(scope='module')
def tracks():
    """200 random tracks per kind, magnitudes 1e-3 .. 1e4, made once."""
    return {kind: psh.random_tracks(kind, N_TRACKS, seed) for seed, kind in enumerate(psh.KINDS)}


def run(exe, kind, tracks, t, tmp_path):
    src, dst = str(tmp_path / f'{kind}.in'), str(tmp_path / f'{kind}.out')
    psh.check_input(kind, tracks).astype('<f8').tofile(src)
    subprocess.run([exe, MODE[kind], float(t).hex(), src, dst], check=True, timeout=60)
    return np.fromfile(dst, f32)


def check_all(exe, tracks, tmp_path):
    for kind in psh.KINDS:
        for t in psh.TIMES:
            got = run(exe, kind, tracks[kind], t, tmp_path)
            want = psh.expected(kind, tracks[kind], t)
            assert got.tobytes() == want.tobytes(), (kind, t)
    # bad arguments: an unknown mode, a t that is no number, records that are not whole
    src = str(tmp_path / 'spheres.in')
    assert subprocess.run([exe, 'box', '0.5', src, src + '.x'], capture_output=True).returncode == 2
    assert subprocess.run([exe, 'sphere', 'nan', src, src + '.x'], capture_output=True).returncode == 2
    assert subprocess.run([exe, 'quad', '0.5', src, src + '.x'], capture_output=True).returncode == 2


def test_inputs_cover_the_magnitudes_and_the_rows_keep_what_the_kernel_does_not_write(tracks):
    for kind in psh.KINDS:
        rec = pose.track_records(tracks[kind])[psh.STORAGE_POS[kind]][1]
        mag = np.abs(rec[:, :6])
        assert rec.shape == (N_TRACKS, pose.REC_DOUBLES[kind]) and mag.min() < 1e-2 and mag.max() > 1e3
        rest = psh.rest_records(tracks[kind])[psh.STORAGE_POS[kind]][0]
        kept = [c for c in range(rest.shape[1]) if c not in psh.CHANGED[kind]]
        for t in (0.0, 1.0 / 3.0, 1.0):
            rows = pose.posed_records(tracks[kind], t)[psh.STORAGE_POS[kind]][1]
            assert rows[:, kept].tobytes() == rest[:, kept].tobytes(), (kind, t)  # r; normal, u, v, w; e1, e2, n
            if t:
                assert rows[:, psh.CHANGED[kind]].tobytes() != rest[:, psh.CHANGED[kind]].tobytes()


def test_check_program_equals_the_python_definition(tracks, tmp_path):
    exe = str(tmp_path / 'pose_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'pose_check', f'POSE_CHECK={exe}'], check=True)
    check_all(exe, tracks, tmp_path)


def test_check_program_under_sanitizers(tracks, tmp_path):
    """The same program built with -fsanitize=address,undefined, stand-alone on the same tracks."""
    exe = str(tmp_path / 'pose_check_san')
    subprocess.run(['make', '-s', '-C', CSRC, 'pose_check', f'POSE_CHECK={exe}',
                    'POSE_CHECK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all -g'], check=True)
    check_all(exe, tracks, tmp_path)


def test_pose_at_zero_is_not_the_rest_row_of_a_negative_zero(tmp_path):
    """Q.x = -0.0: Q + 0.0 * d is +0.0, so the row at t = 0 differs from the compiled row in that sign bit and in
    nothing else. This is why the rest state comes back by unpose(), not by pose(0.0)."""
    exe = str(tmp_path / 'pose_check')
    subprocess.run(['make', '-s', '-C', CSRC, 'pose_check', f'POSE_CHECK={exe}'], check=True)
    q = core.quad(core.vec3(-0.0, 1.0, 2.0), core.vec3(0, 0, 3.0), core.vec3(0, 2.0, 0), psh.MAT)
    tracks = {'quads': {0: (q, core.vec3(1.0, 0.5, 0.25))}}
    rest = psh.rest_records(tracks)[1][0]
    got = run(exe, 'quads', tracks, 0.0, tmp_path)
    assert got.tobytes() == psh.expected('quads', tracks, 0.0).tobytes()
    row0 = rest.copy()
    row0[0, psh.CHANGED['quads']] = got[:4]
    assert np.array_equal(row0, rest)  # equal as numbers
    diff = row0.view(np.uint32) ^ rest.view(np.uint32)
    assert np.flatnonzero(diff).tolist() == [4] and diff[0, 4] == 0x80000000  # Q.x's sign bit alone


def test_the_box_at_t_lies_within_the_union_of_the_boxes_at_both_ends():
    rng = np.random.default_rng(17)
    times = rng.uniform(0.0, 1.0, 50)
    assert times.min() > 0.0 and times.max() < 1.0
    for seed, kind in enumerate(psh.KINDS):
        tracks = psh.random_tracks(kind, 40, 100 + seed)

        def box(t):
            return psh.BOX_RULE[kind](pose.posed_records(tracks, t)[psh.STORAGE_POS[kind]][2])

        (mn0, mx0), (mn1, mx1) = box(0.0), box(1.0)
        lo, hi = np.minimum(mn0, mn1), np.maximum(mx0, mx1)
        for t in times:
            mn, mx = box(float(t))
            assert np.all(mn >= lo) and np.all(mx <= hi), (kind, t)
