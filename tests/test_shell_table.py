"""CPU: the wave-resident shell table (csrc/pt_shell_chain.hpp: shell_table_entry,
the layout kTab*, and shell_chain_begin reading it), run by the `table` mode of
csrc/shell_chain_check.cpp: the table is built into an array of 128 dwords,
lane by lane as the megakernel's prologue does, and the expanded begin and the
skipped shell's finish read that array alone.

Exactness: leaf and t bits of oracle.traverse, 0 mismatches, on the ray sets
of test_shell_chain.py for both vol2 fixtures and for synthetic shells with
chains of 0, 1, 5, 6 and 7 levels (7: six are expanded), chain children on
child 0 only, on child 1 only and mixed, with a wrong hint and without one.
Content: every entry equals the node float it was taken from, bit for bit.
The program built with -fsanitize=address,undefined, run directly, gives the
same output."""
import subprocess

import numpy as np
import pytest

import shell_chain_helpers as ch
import shell_scenes as ss
from parity_helpers import fixture
from ptmi import scene_data as sd
from test_shell_chain import CAM_WIDTH, VOL2, ray_set

f32 = np.float32

# pt_shell_chain.hpp
TAB_SHARED, TAB_LEVEL, TAB_STRIDE = 0, 9, 10
TAB_REST = TAB_LEVEL + TAB_STRIDE * ch.CHAIN_MAX
TAB_LEAF = TAB_REST + 1
TAB_SPHERE = TAB_LEAF + 7
TAB_SIZE = TAB_SPHERE + 4


@pytest.fixture(scope='module')
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp('st')
    return (ch.build_check(str(d / 'shell_chain_check')),
            ch.build_check(str(d / 'shell_chain_check_san'), '-fsanitize=address,undefined -fno-sanitize-recover=all -g'))


def run_table(exe, tmp_path, layout, rays, stack, shell=None):
    """The check program's table mode: (info, table as u32[TAB_SIZE], out as (n, 8) u32)."""
    names = ('nodes', 'spheres', 'quads', 'tris')
    paths = [str(tmp_path / (n + '.f32')) for n in names] + [str(tmp_path / 'rays.f32'), str(tmp_path / 'out.u32')]
    for n, p in zip(names, paths):
        np.ascontiguousarray(getattr(layout, n), f32).tofile(p)
    np.ascontiguousarray(rays, f32).reshape(-1, 7).tofile(paths[4])
    args = [layout.shell if shell is None else shell, layout.n_inner, layout.root_ref, layout.max_leaf_depth, stack]
    r = subprocess.run([exe] + [str(int(a)) for a in args] + paths + ['table'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split('\n')
    w = lines[0].split()
    assert w[0] == 'chain' and w[14] == 'off'
    info = dict(m=int(w[2]), full=int(w[4]), side=int(w[6]), plan_m=int(w[9]), skip=int(w[11]), slots=int(w[13]),
                off=[int(x) for x in w[15:]])
    t = lines[1].split()
    assert t[0] == 'table' and len(t) == 1 + TAB_SIZE
    return info, np.array([int(x, 16) for x in t[1:]], np.uint32), np.fromfile(paths[5], np.uint32).reshape(-1, 8)


def expected_table(layout, info, shell):
    """The table from the node and sphere arrays, by the layout's definition."""
    nodes = np.ascontiguousarray(layout.nodes, f32)
    u = nodes.view(np.uint32)
    t = np.zeros(TAB_SIZE, np.uint32)

    def box(row, c):  # six box floats, cx, cy, cz
        lo_hi = nodes[row, c:12:2]
        cx = (lo_hi[0] + lo_hi[3]) * f32(0.5)
        cy = (lo_hi[1] + lo_hi[4]) * f32(0.5)
        return np.concatenate([lo_hi, [cx, cy, nodes[row, 14 + c]]]).astype(f32).view(np.uint32)

    m = info['plan_m']
    if m > 0:
        rows = [o // sd.NODE_BYTES for o in info['off']]
        side = [(info['side'] >> k) & 1 for k in range(m)]
        t[TAB_SHARED:TAB_SHARED + 9] = box(rows[0], side[0])
        for k in range(m):
            b = TAB_LEVEL + TAB_STRIDE * k
            t[b:b + 9] = box(rows[k], side[k] ^ 1)
            t[b + 9] = u[rows[k], 12 + (side[k] ^ 1)]
        t[TAB_REST] = u[rows[m - 1], 12 + side[m - 1]]
    if shell > 0:
        v = shell - 1
        row, pc = (v & ~1) // sd.NODE_BYTES, v & 1
        t[TAB_LEAF:TAB_LEAF + 6] = u[row, pc:12:2]
        ref = int(u[row, 12 + pc])
        t[TAB_LEAF + 6] = ref
        if ref >> 31 and (ref >> 28) & 3 == sd.PRIM_SPHERE:
            t[TAB_SPHERE:TAB_SPHERE + 4] = np.ascontiguousarray(layout.spheres, f32).view(np.uint32).reshape(-1, 4)[ref & 0x01ffffff]
    return t


def check(exes, tmp_path, sa, cam, n, seed, stack, shell=None, expanded=True):
    import oracle
    layout = sd.pack_device(sa, leaf_order=False)  # device primitive rows = the oracle's indices
    if shell == 'wrong':
        shell = layout.shell ^ 1
    rays, osc = ray_set(sa, cam, n, seed)
    outs = [run_table(exe, tmp_path, layout, rays, stack, shell) for exe in exes]
    info, tab, out = outs[0]
    for other in outs[1:]:  # the sanitizer build: clean, same output
        assert other[0] == info and np.array_equal(other[1], tab) and np.array_equal(other[2], out)
    # the mode without the table array: the same walks
    info0, out0 = ch.run_check(exes[0], tmp_path, layout, rays, stack, shell)
    assert info0 == info and np.array_equal(out0, out)
    want = expected_table(layout, info, layout.shell if shell is None else shell)
    assert np.array_equal(tab, want), np.nonzero(tab != want)[0]
    bad = 0
    for r, res in zip(rays, out):
        hit, t, ty, ix = oracle.traverse(osc, r[:3], r[3:6], float(r[6]))
        ref, tb = int(res[3]), res[4]
        if hit:
            ok = ref != 0 and ((ref >> 28) & 3, ref & 0x01ffffff) == (ty, ix) and tb == f32(t).view(np.uint32)
        else:
            ok = ref == 0
        bad += not ok
    n_exp = int(out[:, 6].sum())
    print(f'{len(rays)} rays, plan m {info["plan_m"]} skip {info["skip"]} side {info["side"]:#b}, {n_exp} began expanded, '
          f'{int(out[:, 7].sum())} tested the skipped shell, {bad} mismatches')
    assert bad == 0
    if expanded:
        assert 0 < n_exp < len(rays)  # both sides of the gate
    else:
        assert info['plan_m'] == 0 and n_exp == 0 and not tab[:TAB_LEAF].any()
    return info, tab, out


@pytest.mark.parametrize('name', VOL2)
def test_table_vol2(exes, tmp_path, name):
    info, tab, out = check(exes, tmp_path, fixture(name), sd.fixture_camera(name, CAM_WIDTH[name]), 900, 41, 20)
    assert (info['plan_m'], info['skip']) == (5, 1) and out[:, 7].sum() > 0
    assert not tab[TAB_LEVEL + 5 * TAB_STRIDE:TAB_REST].any()  # level 5 is not expanded
    # the shell's leaf box is the shared box, bit for bit
    assert np.array_equal(tab[TAB_LEAF:TAB_LEAF + 6], tab[TAB_SHARED:TAB_SHARED + 6])


# levels, flip (bit k: level k's chain child is child 0), levels expanded, skip
CHAINS = [(1, 0b0, 1, 1), (1, 0b1, 1, 1), (5, 0b00000, 5, 1), (5, 0b11111, 5, 1), (5, 0b01101, 5, 1),
          (6, 0b000000, 6, 1), (6, 0b111111, 6, 1), (6, 0b100110, 6, 1), (7, 0b1011001, 6, 0), (7, 0b0000000, 6, 0)]


@pytest.mark.parametrize('R', [100.0, 5000.0])
@pytest.mark.parametrize('length,flip,m,skip', CHAINS)
def test_table_synthetic(exes, tmp_path, length, flip, m, skip, R):
    sa = ch.rechain(ch.chain_arrays('few', R), length, flip)
    layout = sd.pack_device(sa)
    info, tab, _ = check(exes[:1] if R == 100.0 else exes, tmp_path, sa, ss.shell_camera(R, 'inside'), 300, 43,
                         ch.kernel_slots(layout.max_leaf_depth))
    assert (info['plan_m'], info['skip']) == (m, skip)
    assert info['side'] == ~flip & ((1 << m) - 1)  # child 1 unless flipped


@pytest.mark.parametrize('shell', [0, 'wrong'])
def test_table_without_a_chain(exes, tmp_path, shell):
    """A missing hint fills nothing; a wrong hint (the other child of the
    hint's node, an internal node or another leaf) finds no chain, the level
    entries stay 0 and every walk is the ordinary one."""
    sa = ch.scene_arrays('c3', 5000.0)
    _, tab, _ = check(exes, tmp_path, sa, ss.shell_camera(5000.0, 'inside'), 300, 47, 16, shell=shell, expanded=False)
    if shell == 0:
        assert not tab.any()


def test_table_builder_scene(exes, tmp_path):
    """The SAH builder's own five levels (sah5), mixed sides as it chose them."""
    sa = ch.scene_arrays('sah5', 5000.0)
    info, _, _ = check(exes[:1], tmp_path, sa, ss.shell_camera(5000.0, 'inside'), 300, 49,
                       ch.kernel_slots(sd.pack_device(sa).max_leaf_depth))
    assert (info['plan_m'], info['skip']) == (5, 1)
