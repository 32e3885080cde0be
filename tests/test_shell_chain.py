"""CPU: the shell chain (csrc/pt_shell_chain.hpp, the functions the
megakernel's SHELL kernels call, run on the CPU by csrc/shell_chain_check.cpp).

Discovery: the chain of ancestors above the shell's leaf, on both vol2
fixtures, on synthetic scenes with chains of 1, 3, 5 and 8 levels, without a
hint, and on node arrays in which no child or both children carry the box.
Exactness: the expanded walk with its finish returns the leaf and the t bits
of oracle.traverse, 0 mismatches. Slots: no ray's peak stack occupancy exceeds
shell_chain_slots, which on vol2 is the tree's worst case exactly. The
program built with -fsanitize=address,undefined gives the same output."""
import numpy as np
import pytest

import shell_chain_helpers as ch
from parity_helpers import fixture
from ptmi import scene_data as sd

f32 = np.float32
VOL2 = ('vol2_final_scene', 'vol2_final_scene_comparison')
CAM_WIDTH = {VOL2[0]: 800, VOL2[1]: 3840}  # the fixtures' cameras


@pytest.fixture(scope='module')
def check_exe(tmp_path_factory):
    return ch.build_check(str(tmp_path_factory.mktemp('sc') / 'shell_chain_check'))


@pytest.fixture(scope='module')
def san_exe(tmp_path_factory):
    return ch.build_check(str(tmp_path_factory.mktemp('sc_san') / 'shell_chain_check_san'),
                          '-fsanitize=address,undefined -fno-sanitize-recover=all -g')


ONE_RAY = np.array([[0, 0, 0, 1, 0, 0, 0.001]], f32)


# ------------------------------------------------------------------ discovery
@pytest.mark.parametrize('name', VOL2)
def test_vol2_chain(check_exe, tmp_path, name):
    """The issue's table: five levels, the shell's leaf under the fifth; the
    sibling subtrees' leaves and deepest leaves."""
    layout = sd.pack_device(fixture(name))
    info, _ = ch.run_check(check_exe, tmp_path, layout, ONE_RAY, 20)
    assert (info['m'], info['full']) == (5, 1)
    assert info['off'][0] == 0 and info['off'][-1] == (layout.shell - 1) & ~1
    got = []
    for k, off in enumerate(info['off']):
        sib = ((info['side'] >> k) & 1) ^ 1
        leaves, depth = ch.subtree(layout, int(layout.nodes[off // sd.NODE_BYTES, 12 + sib].view(np.int32)))
        got.append((leaves, k + 1 + depth))
    assert got == [(2066, 15), (1180, 15), (121, 12), (38, 11), (2, 6)]
    assert layout.max_leaf_depth == 15
    # the 20-slot kernel expands all five and skips the leaf: 15 + 5 - 1 slots
    assert (info['plan_m'], info['skip'], info['slots']) == (5, 1, 19)
    # the 16-slot kernel has room for one level and the rest of the chain
    info16, _ = ch.run_check(check_exe, tmp_path, layout, ONE_RAY, 16)
    assert (info16['plan_m'], info16['skip'], info16['slots']) == (1, 0, 16)


@pytest.mark.parametrize('name,m,full,plan', [('c1', 1, 1, (1, 1)), ('c3', 3, 1, (3, 1)), ('c8', 6, 0, (6, 0)),
                                              ('sah5', 5, 1, (5, 1)), ('deep', 5, 1, (3, 0))])
def test_synthetic_chains(check_exe, tmp_path, name, m, full, plan):
    layout = sd.pack_device(ch.scene_arrays(name, 100.0))
    assert layout.shell > 0
    stack = ch.kernel_slots(layout.max_leaf_depth)
    info, _ = ch.run_check(check_exe, tmp_path, layout, ONE_RAY, stack)
    assert (info['m'], info['full']) == (m, full)
    if name == 'c8':  # not full: one slot for the rest of the chain, so at most stack - max_leaf_depth levels
        assert layout.max_leaf_depth == 11
        plan = (5, 0)
    assert (info['plan_m'], info['skip']) == plan
    want = layout.max_leaf_depth + plan[0] - plan[1]
    assert info['slots'] == want <= stack
    if name == 'deep':
        assert layout.max_leaf_depth == 17  # the 20-slot kernel: fewer levels than found
    # the chain walks down from the root through internal children
    off = 0
    for k in range(info['m']):
        assert info['off'][k] == off
        off = int(layout.nodes[off // sd.NODE_BYTES, 12 + ((info['side'] >> k) & 1)].view(np.int32))
    if full:
        assert off < 0 and info['off'][-1] == (layout.shell - 1) & ~1


def test_no_hint_and_ambiguous_nodes(check_exe, tmp_path):
    layout = sd.pack_device(ch.scene_arrays('c3', 100.0))
    info, out = ch.run_check(check_exe, tmp_path, layout, ONE_RAY, 16, shell=0)
    assert (info['m'], info['plan_m']) == (0, 0) and out[0, 6] == 0
    # a scene without a shell
    plain = sd.pack_device(fixture('cornell_smoke', 96))
    assert plain.shell == 0
    info, out = ch.run_check(check_exe, tmp_path, plain, ONE_RAY, 16)
    assert (info['m'], info['plan_m']) == (0, 0) and out[0, 6] == 0
    # both children of the root carry the shell's box: no expansion, the ordinary path
    both = sd.pack_device(ch.scene_arrays('c3', 100.0))
    both.nodes = both.nodes.copy()
    side = 0  # c3: the root's chain child is child 1 (flip bit 0 clear)
    both.nodes[0, side:12:2] = both.nodes[0, 1:12:2]
    both.nodes[0, 14 + side] = both.nodes[0, 15]
    info, out = ch.run_check(check_exe, tmp_path, both, ONE_RAY, 16)
    assert (info['m'], info['plan_m']) == (0, 0) and out[0, 6] == 0
    # ... at the second level: one level is expanded, the rest of the chain is pushed
    two = sd.pack_device(ch.scene_arrays('c3', 100.0))
    two.nodes = two.nodes.copy()
    row = int(two.nodes[0, 13].view(np.int32)) // sd.NODE_BYTES
    two.nodes[row, 1:12:2] = two.nodes[row, 0:12:2]  # c3: level 1's chain child is child 0 (flip bit 1)
    two.nodes[row, 15] = two.nodes[row, 14]
    info, _ = ch.run_check(check_exe, tmp_path, two, ONE_RAY, 16)
    assert (info['m'], info['full'], info['plan_m'], info['skip']) == (1, 0, 1, 0)
    # no child carries it (a hint that points at another leaf)
    wrong = sd.pack_device(ch.scene_arrays('c3', 100.0))
    wrong.shell ^= 1  # the other child of the hint's node
    info, out = ch.run_check(check_exe, tmp_path, wrong, ONE_RAY, 16)
    assert (info['m'], info['plan_m']) == (0, 0) and out[0, 6] == 0


# ------------------------------------------------------------------ exactness
def unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def ray_set(sa, cam, n, seed):
    """(o, d, tmin) rows: camera rays; rays scattered from what they hit; exit
    searches (tmin = t_entry + 1e-4) from every medium boundary hit; directions
    within 0 .. 1e-3 of the axes; |d| from 1e-3 to 2; origins inside the gate,
    between the gate and the shell, and outside the shell."""
    import oracle
    osc = oracle.OracleScene(sa)
    rng = np.random.default_rng(seed)
    R = float(sa.sphere_data[:, 3].max())
    rays = []
    # camera rays
    c, p00, du, dv = (np.asarray(cam[k], np.float64) for k in ('center', 'pixel00', 'delta_u', 'delta_v'))
    px = rng.uniform(0, cam['width'], (n // 3, 1))
    py = rng.uniform(0, cam['height'], (n // 3, 1))
    d = p00 + px * du + py * dv - c
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    first = [(c.astype(f32), x.astype(f32), f32(0.001)) for x in d]
    rays += first
    # scattered from the hit points, and exit searches from medium boundaries
    med = sa.sphere_mats['is_constant_medium']
    for o, x, tmin in first:
        hit, t, ty, ix = oracle.traverse(osc, o, x)
        if not hit:
            continue
        if ty == sd.PRIM_SPHERE and med[ix]:
            rays.append((o, x, f32(t) + f32(0.0001)))
        hp = (o + x * f32(t)).astype(f32)
        rays.append((hp, (unit(rng, 1)[0] * rng.choice([1e-3, 0.37, 1.0, 2.0])).astype(f32), f32(0.001)))
    # origins on both sides of the gate, random and near-axis directions at several lengths
    def origin(k):
        r = (0.0, 0.3, 0.499, 0.501, 0.8, 1.2)[k % 6] * R
        return (unit(rng, 1)[0] * r).astype(f32)

    for k in range(n // 3):
        rays.append((origin(k), (unit(rng, 1)[0] * (1e-3, 0.37, 1.0, 2.0)[k % 4]).astype(f32), f32(0.001)))
    k = 0
    for axis in range(3):
        for sign in (1.0, -1.0):
            for eps in (0.0, 1e-9, 1e-7, 1e-5, 1e-3):
                for length in (1e-3, 0.37, 1.0, 2.0):
                    for _ in range(3):
                        x = eps * rng.uniform(-1, 1, 3)
                        x[axis] = sign
                        rays.append((origin(k), (x * length).astype(f32), f32(0.001)))
                        k += 1
    return np.array([np.concatenate([o, x, [t]]) for o, x, t in rays], f32), osc


def check_exact(exes, tmp_path, sa, cam, n, seed, stack):
    import oracle
    layout = sd.pack_device(sa, leaf_order=False)  # device primitive rows = the oracle's indices
    rays, osc = ray_set(sa, cam, n, seed)
    assert len(rays) >= n
    outs = [ch.run_check(exe, tmp_path, layout, rays, stack) for exe in exes]
    info, out = outs[0]
    for other in outs[1:]:
        assert other[0] == info and np.array_equal(other[1], out)  # the sanitizer build: clean, same output
    bad = 0
    for r, res in zip(rays, out):
        hit, t, ty, ix = oracle.traverse(osc, r[:3], r[3:6], float(r[6]))
        for ref, tb in ((int(res[0]), res[1]), (int(res[3]), res[4])):  # the ordinary walk, the expanded one
            if hit:
                ok = ref != 0 and ((ref >> 28) & 3, ref & 0x01ffffff) == (ty, ix) and tb == f32(t).view(np.uint32)
            else:
                ok = ref == 0
            bad += not ok
    n_exp, n_fin = int(out[:, 6].sum()), int(out[:, 7].sum())
    n_exit = int((rays[:, 6] != f32(0.001)).sum())
    print(f'{len(rays)} rays ({n_exit} exit searches), {n_exp} began expanded, {n_fin} tested the skipped shell, '
          f'peak {out[:, 5].max()} of {info["slots"]} slots (ordinary walk: {out[:, 2].max()}), {bad} mismatches')
    assert bad == 0
    assert info['plan_m'] > 0 and 0 < n_exp < len(rays)  # both sides of the gate
    assert (out[:, 5] <= info['slots']).all()
    assert (out[out[:, 6] == 0, 5] <= layout.max_leaf_depth + 1).all()
    return info, rays, out


@pytest.mark.parametrize('name', VOL2)
def test_exact_vol2(check_exe, san_exe, tmp_path, name):
    info, rays, out = check_exact((check_exe, san_exe), tmp_path, fixture(name), sd.fixture_camera(name, CAM_WIDTH[name]), 3000, 21, 20)
    assert info['skip'] == 1 and out[:, 7].sum() > 0
    assert (rays[:, 6] != f32(0.001)).sum() > 20  # exit searches from the r = 70 medium


@pytest.mark.parametrize('stack', [17, 18])
def test_exact_vol2_partial(check_exe, tmp_path, stack):
    """Fewer levels than found, the rest of the chain pushed as a node."""
    info, _, _ = check_exact((check_exe,), tmp_path, fixture(VOL2[0]), sd.fixture_camera(VOL2[0], 800), 3000, 22, stack)
    assert (info['plan_m'], info['skip']) == (stack - 15, 0)


@pytest.mark.parametrize('R', [100.0, 5000.0])
@pytest.mark.parametrize('name', list(ch.SCENES))
def test_exact_synthetic(check_exe, san_exe, tmp_path, name, R):
    import shell_scenes as ss
    sa = ch.scene_arrays(name, R)
    stack = ch.kernel_slots(sd.pack_device(sa).max_leaf_depth)
    check_exact((check_exe, san_exe), tmp_path, sa, ss.shell_camera(R, 'inside'), 1000, 23, stack)


# ---------------------------------------------------------------------- slots
# found by a hill-climbing search over origins inside the gate and directions through vol2's deepest leaves
ADVERSARIAL = [
    (69.23076629638672, 692.8816528320312, 889.8480224609375, -0.16135725378990173, -0.6060863733291626, -0.7788601517677307),
    (75.48384094238281, 701.4075317382812, 894.504638671875, -0.1707662045955658, -0.6073495149612427, -0.77586430311203),
    (35.73112106323242, 590.7675170898438, 753.3906860351562, -0.13961617648601532, -0.609063446521759, -0.7807362079620361),
]


def test_slot_bound_on_vol2(check_exe, tmp_path):
    """The bound is the tree's worst case exactly: with every box hit, the
    near sibling S_k is walked above the m - 1 others and needs (its deepest
    leaf's depth below its root) + 1 slots of its own; the largest of these
    sums is shell_chain_slots. Rays: aimed from inside the gate through the
    deepest leaves, plus three found by search that hit every sibling with S_0
    nearest. No ray exceeds the bound. The best rays reach 17 of the 19 slots
    where the ordinary walk of the same rays reaches 14 of its 16: the m - 2 =
    3 slots that the bound adds to the ordinary walk's are all used, and the
    two slots of slack are the ordinary walk's own (no ray through vol2's
    deepest leaves hits the far child at every level of its path)."""
    sa = fixture(VOL2[0])
    layout = sd.pack_device(sa)
    b = sa.bvh
    depth = sd.leaf_depths(b)
    leaves = np.nonzero(b['bvh_prim_idx'] >= 0)[0]
    deepest = leaves[depth[leaves] == depth[leaves].max()]
    centres = 0.5 * (b['bvh_bbox_min'][deepest].astype(np.float64) + b['bvh_bbox_max'][deepest])
    rng = np.random.default_rng(31)
    rays = [np.array(r + (0.001,)) for r in ADVERSARIAL]
    for c in centres:
        for _ in range(100):
            o = unit(rng, 1)[0] * rng.uniform(0, 2400.0)
            d = c + rng.uniform(-3, 3, 3) - o
            rays.append(np.concatenate([o, d / np.linalg.norm(d), [0.001]]))
    info, out = ch.run_check(check_exe, tmp_path, layout, np.array(rays, f32), 20)
    m = info['plan_m']
    assert (m, info['skip'], info['slots']) == (5, 1, 19)
    worst = 0
    for k, off in enumerate(info['off']):
        sib = ((info['side'] >> k) & 1) ^ 1
        worst = max(worst, (m - 1) + ch.subtree(layout, int(layout.nodes[off // sd.NODE_BYTES, 12 + sib].view(np.int32)))[1] + 1)
    assert worst == info['slots']
    exp = out[:, 6] == 1
    grow = out[exp, 5].astype(int) - out[exp, 2].astype(int)
    print(f'{len(rays)} rays at {len(centres)} deepest leaves: peak {out[exp, 5].max()} of {info["slots"]} expanded, '
          f'{out[:, 2].max()} of 16 ordinary, largest growth on one ray {grow.max()}')
    assert exp[:3].all() and (out[:, 5] <= info['slots']).all() and (out[:, 2] <= 16).all()
    assert np.array_equal(out[:, 0], out[:, 3]) and np.array_equal(out[:, 1], out[:, 4])
    assert grow.max() == m - 2 and out[exp, 5].max() >= 17
