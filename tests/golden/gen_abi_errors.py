#!/usr/bin/env python3
"""Records tests/golden/abi_errors.json: what the C-ABI answers to rejected
arguments and to no-op calls (tests/abi_table.py has the format and the
replay; tests/test_abi_table.py replays it against the built library).

TEST INFRASTRUCTURE ONLY. The table pins the behaviour of one revision, so it
is recorded from that revision's library and then must be reproduced, byte for
byte, by every later one:

    bash tools/build_ref_variant.sh <rev> parent
    PTMI_LIB=path-tracer-python_amd/ptmi/_lib/variants/libptmi_parent.so \\
        python tests/golden/gen_abi_errors.py

(PTMI_LIB unset: the in-tree library; ``--check`` compares with the committed
file and writes nothing.) It was recorded from the last revision whose
pt_abi.hip spelt every entry point out on its own.

Every case leaves at least one argument rejected or one no-op condition true,
so by that revision's pt_abi.hip it returns before the first HIP call: each
entry point there is a run of ``if (...) return`` lines over the arguments, the
two structs and the host-only size functions (mk_workspace_bytes,
wf_workspace_bytes, mk_max_batch, mk_tile_count), and only the statement
after the last of them launches or calls the runtime. Fully valid calls are
not in the table. No pointer is dereferenced before that point either.

The cases of an entry point come from its STAGES: its checks and no-op
returns in the order the code has them, each with the argument changes that
trip it (the first is the stage's representative). Recorded are
  * every change of every stage alone, so each check, scene and frame checks
    included, is the first failing one of a case of every entry point that
    reaches it;
  * every two neighbouring stages tripped together, which pins their order
    (the no-op returns against the workspace checks included).
to_dev_scene's and to_dev_frame's own inner order is pinned once, through
ptmi_scene_check and ptmi_clear.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, 'path-tracer-python_amd'), os.path.join(ROOT, 'tests')]

import abi_table  # noqa: E402
from ptmi import _lib  # noqa: E402

# A 3-sphere scene that passes ptmi_scene_check, and the empty scene.
SCENE = dict(num_spheres=3, n_inner=2, max_leaf_depth=2, num_bvh_nodes=5, nodes=16, spheres=32, mats=48,
             perlin_vec=64, perlin_perm=80)
# 16 x 8, the whole image, one band: 128 pixels in 2 tiles of 8 x 8.
FRAME = dict(width=16, height=8, x0=0, y0=0, w=16, h=8, band_rows=1, band_stride=1, band_offset=0, max_depth=50)
NO_ROWS = dict(FRAME, h=1, band_stride=2, band_offset=1)  # row 0 belongs to the other rank

# to_dev_scene's checks in order: changes of SCENE that fail each first.
SCENE_STAGES = [
    ('null', [None]),
    ('negative', [dict(num_quads=-1), dict(n_inner=-1)]),
    ('total', [dict(num_spheres=0x10000000)]),
    ('per-type', [dict(num_spheres=(1 << 25) + 1)]),
    ('n_inner', [dict(n_inner=1)]),
    ('nodes', [dict(nodes=0), dict(nodes=24)]),
    ('spheres', [dict(spheres=0), dict(spheres=8)]),
    ('quads', [dict(num_quads=1, n_inner=3, num_bvh_nodes=7), dict(num_quads=1, n_inner=3, num_bvh_nodes=7, quads=4)]),
    ('tris', [dict(num_triangles=1, n_inner=3, num_bvh_nodes=7),
              dict(num_triangles=1, n_inner=3, num_bvh_nodes=7, tris=40)]),
    ('mats', [dict(mats=0), dict(mats=56)]),
    ('perlin', [dict(perlin_vec=0), dict(perlin_vec=72), dict(perlin_perm=0)]),
    ('num_images', [dict(num_images=-1), dict(num_images=17)]),
    ('texels', [dict(num_images=1)]),
    ('leaf-depth-sign', [dict(max_leaf_depth=-1)]),
    ('leaf-depth-ref', [dict(max_leaf_depth=63)]),
    ('num_bvh_nodes', [dict(num_bvh_nodes=4)]),
    ('ref_nodes', [dict(ref_nodes=24)]),
]
# to_dev_frame's checks in order: changes of FRAME.
FRAME_STAGES = [
    ('null', [None]),
    ('window', [dict(w=17), dict(width=0), dict(height=-8), dict(h=0), dict(x0=-1), dict(y0=-1), dict(x0=4, w=13),
                dict(y0=4, h=5)]),
    ('too-large', [dict(width=40000, height=40000)]),
    ('band', [dict(band_rows=0), dict(band_stride=0), dict(band_offset=-1), dict(band_stride=2, band_offset=2)]),
    ('max_depth', [dict(max_depth=300), dict(max_depth=-1)]),
    ('traversal', [dict(traversal=2), dict(traversal=-1)]),
]
STACKLESS = ('stackless', [dict(frame=dict(FRAME, traversal=1))])  # SCENE has nodes and no ref_nodes

MK_NEED_1, MK_NEED_2 = 128 * 12 + 2048, 128 * 24 + 2048  # mk_workspace_bytes(128 pixels, 1 and 2 samples)
MK_MAX_BATCH = (2 ** 32 - 1) // (8 * 64)  # 2 tiles padded to 8 shards' units of 64 items

ACCUM = ('accum', [dict(accum=0)])
STATS = ('stats', [dict(stats=0), dict(stats=40)])
NOOP_ROWS = ('no-rows', [dict(frame=NO_ROWS)])


def workspace(need, bad_size=64):
    return ('workspace', [dict(ws=0), dict(ws=264), dict(ws_bytes=need - 1), dict(ws_bytes=bad_size)])


def entry_points(wf_need):
    """name -> (parameters, good values, stages after the scene / frame ones)."""
    render_ws = ['scene', 'frame', 'ws', 'ws_bytes', 'accum', 's0', 'sc', 'counters', 'stream']
    good = dict(scene=SCENE, frame=FRAME, ws=256, ws_bytes=1 << 40, accum=16, stats=32, out=48, s0=0, sc=2,
                counters=0, stream=0, tl=64, nt=1)
    range0 = ('sample-range', [dict(s0=-1), dict(sc=-1)])  # renders: zero samples are a no-op
    range1 = ('sample-range', [dict(s0=-1), dict(sc=0), dict(sc=-2)])  # one batch: at least one sample
    noop_sc = ('zero-samples', [dict(sc=0)])
    capacity = ('batch-capacity', [dict(sc=MK_MAX_BATCH + 1)])
    count1 = ('sample_count', [dict(sc=0)])
    tonemap_bad = ('arguments', [dict(accum=0), dict(out=0), dict(w=0), dict(h=-1)])
    too_large = ('too-large', [dict(w=40000, h=40000)])
    tm_good = dict(good, w=4, h=4, spp=1)
    frame_only = dict(good, batch=1)
    grid_good = dict(good, tw=64, th=128, tx=192, ty=256)
    upd_good = dict(good, thr='0.05', lo=4, hi=16, state=64, terr=128, tl=192, na=256)
    return {
        'ptmi_scene_check': (['scene'], good, []),
        'ptmi_mk_render': (['scene', 'frame', 'accum', 's0', 'sc', 'counters', 'stream'], good,
                           [ACCUM, range0, ('zero-samples-or-no-rows', [dict(sc=0), dict(frame=NO_ROWS)])]),
        'ptmi_mk_workspace_bytes': (['frame', 'batch'], frame_only, [('batch', [dict(batch=0), dict(batch=-3)])]),
        'ptmi_mk_render_ws': (render_ws, good, [ACCUM, range0, NOOP_ROWS, workspace(MK_NEED_1), noop_sc]),
        'ptmi_mk_trace_ws': (['scene', 'frame', 'ws', 'ws_bytes', 's0', 'sc', 'counters', 'stream'], good,
                             [range1, NOOP_ROWS, capacity, workspace(MK_NEED_2)]),
        'ptmi_mk_max_batch': (['frame'], good, []),
        'ptmi_mk_resolve_ws': (['frame', 'ws', 'ws_bytes', 'accum', 'sc', 'stream'], good,
                               [ACCUM, count1, NOOP_ROWS, workspace(MK_NEED_2)]),
        'ptmi_wf_workspace_bytes': (['frame', 'batch'], frame_only,
                                    [('batch', [dict(batch=0), dict(batch=-3)]), ('capacity', [dict(batch=1 << 24)])]),
        'ptmi_wf_render': (render_ws, good, [ACCUM, range0, NOOP_ROWS, workspace(wf_need), noop_sc]),
        'ptmi_wf_set_drain_at': (['divisor'], dict(divisor=0), [('divisor', [dict(divisor=-1)])]),
        'ptmi_clear': (['frame', 'accum', 'stream'], good, [ACCUM, NOOP_ROWS]),
        'ptmi_tonemap': (['accum', 'out', 'w', 'h', 'spp', 'stream'], tm_good, [tonemap_bad, too_large]),
        'ptmi_mk_tile_grid': (['frame', 'tw', 'th', 'tx', 'ty'], grid_good,
                              [('outputs', [dict(tw=0), dict(th=0), dict(tx=0), dict(ty=0)])]),
        'ptmi_stats_clear': (['frame', 'stats', 'stream'], good, [STATS, NOOP_ROWS]),
        'ptmi_mk_trace_tiles_ws': (['scene', 'frame', 'ws', 'ws_bytes', 'tl', 'nt', 's0', 'sc', 'counters', 'stream'],
                                   good,
                                   [range1, ('n_tiles', [dict(nt=-1), dict(nt=3)]),
                                    ('tile_list', [dict(tl=0), dict(tl=66)]),
                                    # a frame without rows has no tiles: only an empty list passes the count check
                                    ('no-rows', [dict(frame=NO_ROWS, nt=0), dict(frame=NO_ROWS)]), capacity,
                                    workspace(MK_NEED_2), ('empty-list', [dict(nt=0), dict(nt=0, tl=0)])]),
        'ptmi_mk_resolve_stats_ws': (['frame', 'ws', 'ws_bytes', 'accum', 'stats', 'tl', 'nt', 'sc', 'stream'], good,
                                     [ACCUM, STATS, count1,
                                      ('tile_list', [dict(tl=66), dict(nt=-1), dict(nt=3)]),
                                      ('no-rows', [dict(frame=NO_ROWS, tl=0), dict(frame=NO_ROWS, nt=0),
                                                   dict(frame=NO_ROWS)]),
                                      workspace(MK_NEED_2), ('empty-list', [dict(nt=0)])]),
        'ptmi_wf_render_stats': (render_ws[:5] + ['stats'] + render_ws[5:], good,
                                 [ACCUM, STATS, range0, NOOP_ROWS, workspace(wf_need), noop_sc]),
        'ptmi_tile_update': (['frame', 'stats', 'thr', 'lo', 'hi', 'state', 'terr', 'tl', 'na', 'stream'], upd_good,
                             [STATS, ('threshold', [dict(thr='-0.5'), dict(thr='nan')]),
                              ('spp', [dict(lo=-1), dict(lo=8, hi=4)]),
                              ('buffers', [{k: v} for k in ('state', 'terr', 'tl', 'na') for v in (0, 66)])]),
        'ptmi_tonemap_stats': (['accum', 'stats', 'out', 'w', 'h', 'stream'], tm_good, [tonemap_bad, STATS, too_large]),
        'ptmi_prof_start': (['n'], dict(n=0), [('max_launches', [dict(n=-1)])]),
        'ptmi_prof_stop': (['ms', 'cnt', 'n'], dict(ms=16, cnt=32, n=7),
                           [('arguments', [dict(ms=0), dict(cnt=0), dict(n=-1)])]),
        'ptmi_prof_stop_busy': (['ms', 'busy', 'cnt', 'n'], dict(ms=16, busy=0, cnt=32, n=7),
                                [('arguments', [dict(ms=0), dict(cnt=0), dict(n=-1), dict(busy=48, n=-1)])]),
    }


def struct_stage(param, base, stages):
    """The stages of a struct argument as changes of the call's arguments."""
    return [(f'{param}:{label}', [{param: (None if c is None else dict(base, **c))} for c in changes])
            for label, changes in stages]


def encode(name, value):
    if name in ('scene', 'frame'):
        return None if value is None else {name: {k: v for k, v in value.items() if v != 0}}
    if name == 'thr':
        return {'f': value}
    if name in ('tw', 'th', 'tx', 'ty'):
        return {'i32p': value}
    if name in ('s0', 'sc', 'nt', 'w', 'h', 'spp', 'batch', 'divisor', 'lo', 'hi', 'n', 'ws_bytes'):
        return value
    return value or None  # a pointer


def cases():
    lib = _lib.load()
    fr = abi_table._struct(_lib.Frame, FRAME)
    import ctypes as C
    wf_need = int(lib.ptmi_wf_workspace_bytes(C.byref(fr), 1))
    assert wf_need > 64
    for fn, (params, good, own) in entry_points(wf_need).items():
        stages = []
        if 'scene' in params:
            stages += struct_stage('scene', SCENE, SCENE_STAGES)
        if 'frame' in params:
            stages += struct_stage('frame', FRAME, FRAME_STAGES)
        if 'scene' in params and 'frame' in params:
            stages.append(STACKLESS)
        stages += own
        changes = [c for _, cs in stages for c in cs]
        inner = fn in ('ptmi_scene_check', 'ptmi_clear')  # the structs' inner order, once
        for (la, a), (lb, b) in zip(stages, stages[1:]):
            if la.split(':')[0] == lb.split(':')[0] and ':' in la and not inner:
                continue
            if set(a[0]) & set(b[0]):  # both stages change the same argument: merge struct fields
                (k,) = set(a[0]) & set(b[0])
                if a[0][k] is None or b[0][k] is None or not isinstance(a[0][k], dict):
                    continue
                base = SCENE if k == 'scene' else FRAME
                both = dict(a[0][k], **{f: v for f, v in b[0][k].items() if base.get(f, 0) != v})
                changes.append({**a[0], **b[0], k: both})
            else:
                changes.append(dict(a[0], **b[0]))
        for c in changes:
            assert c, fn  # a fully valid call would reach the device
            vals = dict(good, **c)
            yield fn, [encode(p, vals[p]) for p in params]


def record():
    lib = _lib.load()
    out, seen = [], set()
    for fn, args in cases():
        key = json.dumps([fn, args])
        if key in seen:
            continue
        seen.add(key)
        ret, err = abi_table.call(lib, fn, args)
        out.append({'fn': fn, 'args': args, 'ret': ret, 'err': err})
    return '[\n' + ',\n'.join(json.dumps(c) for c in out) + '\n]\n'


if __name__ == '__main__':
    text = record()
    if '--check' in sys.argv:
        with open(abi_table.TABLE) as f:
            same = f.read() == text
        print('identical' if same else 'DIFFERENT', abi_table.TABLE)
        sys.exit(0 if same else 1)
    with open(abi_table.TABLE, 'w') as f:
        f.write(text)
    print(f'{text.count(chr(10)) - 2} cases -> {abi_table.TABLE}')
