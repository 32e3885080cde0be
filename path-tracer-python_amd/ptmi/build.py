"""ctypes binding of the device-build ABI (include/ptmi_build.h): the binned-SAH
builder of ``bvh.build_sah`` run on the device, bit for bit, and the packer of
its arrays into a resident scene's tensors.

The entry points live in the same libptmi.so as the integrator's and are loaded
through ``_lib.load()``; their signature table is kept here and bound by
``_lib.bind``.

``DeviceScene.rebuild(builder='device')`` (ptmi.device) is the caller;
``DeviceBuilder`` holds the device buffers of one scene's builds, and
``layout_of`` is the host half: the DeviceLayout of what the pack left on the
device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .scene_data import BVH_KEYS, ByCode, DeviceLayout, KINDS, STORAGE

BUILD_VERSION = 1  # PTMI_BUILD_VERSION of include/ptmi_build.h
MAX_PRIMS = 4096  # PTMI_BUILD_MAX_PRIMS
LANES = 1024  # PTMI_BUILD_LANES
SORT_MAX = 1024  # PTMI_BUILD_SORT_MAX
STATUS_WORDS, INFO_WORDS = 8, 12
NEEDS_HOST = 1  # PTMI_BUILD_NEEDS_HOST
PACK_SKIPPED, PACK_REJECTED = 1, 2

# The mean growth above which update_primitives(rebuild='auto', builder='device')
# rebuilds: tree.REBUILD_GROWTH's rule with the device rebuild's wall time in the
# host rebuild's place (profiles/device_build/policy.json: vol2 on one MI355X,
# rebuild_bvh(builder='device') 11.65 ms against 8.89 ms on the host, so the
# +-50 % scatter, growth 3.895, which saves 9.05 ms per step, no longer pays
# within one step, and the +-100 % scatter, growth 10.84, saving 34 ms, is the
# first that does). Just below that sweep point's growth, so that the point
# itself rebuilds. The device path is the slower one today:
# the threshold is higher than the host's, not lower.
REBUILD_GROWTH_DEVICE = 10.83


class BuildArrays(C.Structure):
    """ptmi_build_arrays."""
    _fields_ = [(k, C.c_void_p) for k in ('bbox_min', 'bbox_max', 'left', 'right', 'parent', 'prim_type', 'prim_idx')]


class BuildMaps(C.Structure):
    """ptmi_build_maps: one int32 array per type code."""
    _fields_ = [(k.name, C.c_void_p) for k in KINDS]


def _signatures():
    """Every export of include/ptmi_build.h: name -> (restype, argtypes)."""
    P, I, Z = C.c_void_p, C.c_int32, C.c_size_t
    A, M = C.POINTER(BuildArrays), C.POINTER(BuildMaps)
    return {
        'ptmi_build_workspace_bytes': (Z, [I]),
        'ptmi_build_sah_device': (C.c_int, [P, I, P, I, P, I, A, P, P, Z, P]),
        'ptmi_build_pack': (C.c_int, [C.POINTER(_lib.SceneView), A, P, M, M, M, P, P, Z, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the build exports bound; a library
    without them raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


def workspace_bytes(n_prims):
    return int(load().ptmi_build_workspace_bytes(int(n_prims)))


def builder_records(sa):
    """(spheres, quads, tris) of a SceneArrays in the builder's form: {c, r}; {Q, u, v}; {v0, v1, v2}."""
    q, t = sa.quads, sa.tris
    return (np.ascontiguousarray(sa.sphere_data, np.float32).reshape(-1, 4),
            np.concatenate([q['quad_Q'], q['quad_u'], q['quad_v']], axis=1).astype(np.float32).reshape(-1, 9),
            np.concatenate([t['triangle_v0'], t['triangle_v1'], t['triangle_v2']], axis=1).astype(np.float32)
            .reshape(-1, 9))


class DeviceBuilder:
    """The device buffers of ptmi_build_sah_device and ptmi_build_pack for
    ``counts`` (ByCode) primitives on ``device``, allocated once: the records,
    the seven arrays, status and info, the maps and the workspace, as slices
    of one int32 and one float32 tensor."""

    def __init__(self, counts, device):
        import torch
        self.counts = ByCode(*(int(c) for c in counts))
        self.n = n = sum(self.counts)
        if not 0 < n <= MAX_PRIMS:
            raise _lib.PtmiError(f'the device builder takes 1 to {MAX_PRIMS} primitives, not {n}')
        self.device = device
        self.nodes = nn = 2 * n - 1
        ns, nt, nq = self.counts
        self.ws_bytes = workspace_bytes(n)
        # float words: records (spheres, quads, tris), bbox_min, bbox_max
        self.f_off = np.cumsum([0, 4 * ns, 9 * nq, 9 * nt, 3 * nn, 3 * nn])
        # int words: left, right, parent, prim_type, prim_idx, status, info, then old_row, new_row, perm by type code
        self.i_off = np.cumsum([0, nn, nn, nn, nn, nn, STATUS_WORDS, INFO_WORDS] + [ns, nt, nq] * 3)
        # empty, not zeros: a fill on the allocating stream would be unordered with an upload on another, and every
        # word that is read has been uploaded or written by a kernel before
        self.tf = torch.empty(int(self.f_off[-1]) + 4, dtype=torch.float32, device=device)
        self.ti = torch.empty(int(self.i_off[-1]) + 4, dtype=torch.int32, device=device)
        self.ws = torch.empty(self.ws_bytes // 4 + 4, dtype=torch.int32, device=device)
        pf, pi = self.tf.data_ptr(), self.ti.data_ptr()
        fp = [pf + 4 * int(o) for o in self.f_off]
        ip = [pi + 4 * int(o) for o in self.i_off]
        self.rec_ptr = fp[0:3]
        self.arrays = BuildArrays(fp[3], fp[4], *ip[0:5])
        self.status_ptr, self.info_ptr = ip[5], ip[6]
        self.old_row, self.new_row, self.perm = (BuildMaps(*ip[7 + 3 * j:10 + 3 * j]) for j in range(3))

    def upload(self, records, old_row):
        """The builder-form ``records`` (spheres, quads, tris) and the ByCode ``old_row`` maps (reference index ->
        device row), in two copies on the current stream."""
        import torch
        f = np.concatenate([np.ascontiguousarray(r, np.float32).reshape(-1) for r in records])
        i = np.concatenate([np.asarray(m, np.int64).astype(np.int32).reshape(-1) for m in old_row])
        self.tf[:f.size].copy_(torch.from_numpy(f), non_blocking=False)
        a = int(self.i_off[7])
        self.ti[a:a + i.size].copy_(torch.from_numpy(i), non_blocking=False)

    def build(self, stream_ptr):
        ns, nt, nq = self.counts
        lib = load()
        _lib.check(lib.ptmi_build_sah_device(self.rec_ptr[0], ns, self.rec_ptr[1], nq, self.rec_ptr[2], nt,
                                             C.byref(self.arrays), self.status_ptr, self.ws.data_ptr(), self.ws_bytes,
                                             stream_ptr), 'ptmi_build_sah_device')

    def pack(self, view, stream_ptr):
        _lib.check(load().ptmi_build_pack(view, C.byref(self.arrays), self.status_ptr, C.byref(self.old_row),
                                          C.byref(self.new_row), C.byref(self.perm), self.info_ptr,
                                          self.ws.data_ptr(), self.ws_bytes, stream_ptr), 'ptmi_build_pack')

    def read_ints(self):
        """(bvh int arrays by key, status, info, new_row ByCode, perm ByCode) read back in one copy."""
        w = self.ti.cpu().numpy()
        o = [int(x) for x in self.i_off]
        part = [w[o[j]:o[j + 1]] for j in range(len(o) - 1)]
        ints = dict(zip(BVH_KEYS[2:], part[0:5]))
        return ints, part[5], part[6], ByCode(*part[10:13]), ByCode(*part[13:16])

    def read_boxes(self):
        w = self.tf.cpu().numpy()
        o = [int(x) for x in self.f_off]
        return w[o[3]:o[4]].reshape(-1, 3), w[o[4]:o[5]].reshape(-1, 3)

    def read_bvh(self):
        """The seven arrays as ``bvh.build_sah`` returns them, and the status block."""
        ints, status, _, _, _ = self.read_ints()
        bmin, bmax = self.read_boxes()
        out = {'bvh_bbox_min': bmin.copy(), 'bvh_bbox_max': bmax.copy()}
        out.update({k: v.copy() for k, v in ints.items()})
        return out, status.copy()


def layout_of(old: DeviceLayout, tensors, info, perm, shell):
    """The DeviceLayout of a packed scene: ``tensors`` maps nodes, ref_nodes, spheres, quads, tris and mats to the
    device tensors' contents (flat numpy), ``info`` is the pack's block, ``perm`` its ByCode new device row ->
    reference index, ``shell`` the hint; everything else is ``old``'s."""
    import dataclasses
    shaped = {k: np.array(tensors[k][:getattr(old, k).size]).reshape(getattr(old, k).shape)
              for k in ('nodes', 'ref_nodes', 'mats') + tuple(k.rows for k in STORAGE)}
    fl = np.asarray(info, np.int32).view(np.float32)
    return dataclasses.replace(old, root_ref=int(info[0]), max_leaf_depth=int(info[1]), root_min=fl[4:7].copy(),
                               root_max=fl[7:10].copy(), prim_perm=ByCode(*(np.asarray(p, np.int64) for p in perm)),
                               n_internal=int(info[2]), shell=int(shell), **shaped)
