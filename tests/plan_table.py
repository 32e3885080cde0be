"""What the C-ABI shows of a launch's shape (test infrastructure only): the
cases of tests/golden/plan_sizes.json, written by tests/golden/gen_plan_sizes.py
from the library of the commit before the launch plans moved into
pt_mk_plan.hpp / pt_wf_plan.hpp. Every call here returns before the library's
first HIP call, so no GPU is needed; pointers are small integers that are never
dereferenced, but for ptmi_mk_tile_grid's four outputs.

A case is {"frame": fields of a ptmi_frame (zero otherwise), "grid": [tile_w,
tile_h, tiles_x, tiles_y], "max_batch", "batches": one entry per batch size
{"batch", "mk": [bytes, err], "wf": [bytes, err]}, "trace": the answers [ret,
err] of ptmi_mk_trace_ws to max_batch + 1 samples (refused: item ids) and to
max_batch samples in a 16-byte workspace (refused with the size it needs)}.
``err`` is ptmi_last_error() after the call, abi_table.SENTINEL if it set none."""
import ctypes as C
import json
import os

import abi_table
from ptmi import _lib

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'plan_sizes.json')
# a scene that passes the argument checks (gen_abi_errors.SCENE)
SCENE = dict(num_spheres=3, n_inner=2, max_leaf_depth=2, num_bvh_nodes=5, nodes=16, spheres=32, mats=48,
             perlin_vec=64, perlin_perm=80)


def answer(lib, frame, batches):
    """The case of one frame: frame is the dict of its non-zero fields."""
    fr = {'frame': frame}
    out = (C.c_int32 * 4)()
    ptr = [C.cast(C.byref(out, 4 * k), C.POINTER(C.c_int32)) for k in range(4)]
    keep = []
    rc = lib.ptmi_mk_tile_grid(abi_table._arg(fr, keep), *ptr)
    assert rc == 0, rc
    max_batch, _ = abi_table.call(lib, 'ptmi_mk_max_batch', [fr])
    case = {'frame': frame, 'grid': list(out), 'max_batch': max_batch, 'batches': []}
    for b in batches + [max_batch, max_batch + 1]:
        case['batches'].append({'batch': b,
                                'mk': list(abi_table.call(lib, 'ptmi_mk_workspace_bytes', [fr, b])),
                                'wf': list(abi_table.call(lib, 'ptmi_wf_workspace_bytes', [fr, b]))})
    case['trace'] = [list(abi_table.call(lib, 'ptmi_mk_trace_ws', [{'scene': SCENE}, fr, 256, ws_bytes, 0, sc, None, None]))
                     for ws_bytes, sc in ((1 << 60, max_batch + 1), (16, max_batch))]
    return case


def load_table():
    with open(TABLE) as f:
        return json.load(f)
