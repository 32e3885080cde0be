"""Device residency of a packed scene and thin wrappers over the C-ABI.

PyTorch is used only as the device allocator / stream provider: every array
of the packed layout (scene_data.DeviceLayout) becomes one torch tensor on
the GPU and the C-ABI receives raw pointers (include/ptmi.h). This replaces
the reference's module-global Taichi fields (fields.py) with a per-device
object, so several scenes can coexist in one process.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np
import torch

from . import (_lib, build as build_mod, bvh as bvh_mod, guide, material, motion, pose as pose_mod, post,
               rigid as rigid_mod, temporal, tree, update, validate, wf_tiles)
from .scene_data import (BVH_KEYS, ByCode, ByStorage, DeviceLayout, KINDS, PRIM_SPHERE, STORAGE, SceneArrays,
                         camera_upload, counts_by_code, find_shell, node_slots, pack_device, shell_hint)


def _stream_or_current(stream, device=None):
    return stream if stream is not None else torch.cuda.current_stream(device)


def _stream_ptr(stream=None, device=None):
    if stream is not None and device is not None and stream.device != device:
        raise _lib.PtmiError(f'stream is on {stream.device}, the scene on {device}')
    return C.c_void_p(_stream_or_current(stream, device).cuda_stream)


def _list_args(cls, lists):
    """A call's three list arguments in storage order from its ``{type code: (pointers..., count)}`` tuples:
    ``byref`` of the ctypes list ``cls``, None for a kind that is missing or empty."""
    return [C.byref(cls(*e)) if e is not None and e[-1] else None for e in (lists.get(k.code) for k in STORAGE)]


def require_gpu():
    if not torch.cuda.is_available():
        raise _lib.PtmiError('no GPU visible: the MI355X integrator has no CPU fallback')
    _lib.load()


class DeviceScene:
    """A packed scene resident in HBM plus its ptmi_scene_view."""

    def __init__(self, scene, device=None):
        require_gpu()
        node_bytes = int(_lib.load().ptmi_node_bytes())
        # PTMI_PACK_LEAF_ORDER=0: compile-order primitives (A/B timing only: same results)
        leaf_order = os.environ.get('PTMI_PACK_LEAF_ORDER', '1') != '0'
        layout = scene if isinstance(scene, DeviceLayout) else pack_device(scene, node_bytes, leaf_order)
        if layout.n_inner and layout.nodes.shape[1] * 4 != node_bytes:
            raise _lib.PtmiError(f'scene packed with {layout.nodes.shape[1] * 4}-B nodes, '
                                 f'libptmi expects {node_bytes}')
        self.layout = layout
        # the reference-layout arrays the scene was packed from: update_primitives keeps them equal to the device
        self.arrays = scene if isinstance(scene, SceneArrays) else None
        self._upd = None  # update_primitives' topology, index maps and root box, made by its first call
        self._tree = None  # tree_growth's baseline areas and result slot, made by its first call
        self._pack = (node_bytes, leaf_order)  # rebuild packs as the scene was packed
        self._builder = None  # rebuild(builder='device')'s device buffers, made by its first call
        self.last_rebuild = None  # {'builder': 'host' | 'device', 'reason': ...} of the last rebuild
        self._tracks = None  # set_tracks' resident tracks, rest edit list, shutter range and posed shell hint
        self.posed = None  # the time pose() last put the tracked primitives at; None: the rest scene
        dev = torch.device(device if device is not None else 'cuda')
        if dev.type != 'cuda':
            raise _lib.PtmiError(f'DeviceScene needs a cuda device, got {dev}')
        # a bare 'cuda' means the current device; fixed here so every later
        # launch goes to the device that holds the scene (the C-ABI launches on
        # the current HIP device)
        self.device = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())

        def up(a):
            a = np.ascontiguousarray(a)
            if a.size == 0:
                a = np.zeros(4, dtype=a.dtype)  # keep a valid 16-B aligned pointer
            return torch.from_numpy(a.reshape(-1).copy()).to(self.device)

        v = _lib.SceneView()
        self.t_nodes = up(layout.nodes)
        for k in STORAGE:  # t_spheres, t_quads, t_tris
            setattr(self, k.tensor, up(getattr(layout, k.rows)))
            setattr(v, k.rows, getattr(self, k.tensor).data_ptr())
            setattr(v, k.count, getattr(layout, k.count))
        self.t_mats = up(layout.mats)
        self.t_texels = up(layout.texels.view(np.int32))
        self.t_pvec = up(layout.perlin_vec)
        self.t_perm = up(layout.perlin_perm)
        self.t_ref_nodes = up(layout.ref_nodes) if layout.ref_nodes is not None else None
        v.nodes = self.t_nodes.data_ptr()
        v.n_inner = layout.n_inner
        v.mats = self.t_mats.data_ptr()
        v.texels = self.t_texels.data_ptr()
        v.num_images = len(layout.img_w)
        for k in range(len(layout.img_w)):
            v.img_offset[k] = layout.img_offset[k]
            v.img_w[k] = layout.img_w[k]
            v.img_h[k] = layout.img_h[k]
        v.perlin_vec = self.t_pvec.data_ptr()
        v.perlin_perm = self.t_perm.data_ptr()
        if self.t_ref_nodes is not None:
            v.ref_nodes = self.t_ref_nodes.data_ptr()
        v.num_bvh_nodes = layout.num_bvh_nodes if layout.ref_nodes is not None else \
            (2 * (layout.n_inner + 1) - 1 if sum(counts_by_code(layout)) else 0)
        self.view = v
        self._set_tree(layout)

    def _set_tree(self, lay):
        """The view's tree fields (root ref, leaf depth, root box, shell hint) from a layout, and the view checked."""
        v = self.view
        v.root_ref, v.max_leaf_depth, v.shell = lay.root_ref, lay.max_leaf_depth, int(lay.shell)
        v.root_min[:], v.root_max[:] = [float(x) for x in lay.root_min], [float(x) for x in lay.root_max]
        _lib.check(_lib.load().ptmi_scene_check(v), 'ptmi_scene_check')

    @classmethod
    def from_arrays(cls, sa: SceneArrays, device=None):
        return cls(sa, device)

    def primitive_rows(self, stream=None):
        """Device-to-device copies of the sphere, quad and triangle row tensors,
        a ByStorage ``(spheres, quads, tris)``: the "previous rows" of a
        motion-aware reprojection (Integrator.reproject_moved), taken before an
        update. Asynchronous on ``stream``."""
        self._require_unposed()
        with torch.cuda.device(self.device), torch.cuda.stream(_stream_or_current(stream, self.device)):
            return ByStorage(*(getattr(self, k.tensor).clone() for k in STORAGE))

    # ------------------------------------------------ scene updates (ptmi.update)
    def _update_state(self):
        """Topology arrays, index maps and the mirror of update_primitives, made once."""
        if self._upd is not None:
            return self._upd
        sa, lay = self.arrays, self.layout
        if sa is None or len(lay.prim_perm) != 3:
            raise _lib.PtmiError('update_primitives needs a DeviceScene made from SceneArrays (it maps reference '
                                 'primitive indices and keeps the arrays equal to the device)')
        if self.t_ref_nodes is None:
            raise _lib.PtmiError('update_primitives needs the scene\'s ref_nodes')
        # the mirror: the geometry, the materials and the boxes are copied, so the caller's arrays stay as they were
        b = dict(sa.bvh, bvh_bbox_min=sa.bvh['bvh_bbox_min'].copy(), bvh_bbox_max=sa.bvh['bvh_bbox_max'].copy())
        self.arrays = sa = dataclasses.replace(sa, sphere_data=sa.sphere_data.copy(), bvh=b,
                                               quads={k: v.copy() for k, v in sa.quads.items()},
                                               tris={k: v.copy() for k, v in sa.tris.items()},
                                               **{k.materials: {key: v.copy() for key, v in sa.mats(k.code).items()}
                                                  for k in KINDS})
        for name in ('nodes', 'spheres', 'quads', 'tris', 'mats', 'ref_nodes', 'root_min', 'root_max'):
            setattr(lay, name, np.array(getattr(lay, name)))  # the layout is refreshed in place: its own copy
        self._tree_state()  # the growth baseline is the tree as built: taken before the first update moves a box
        self._upd = self._topology_state()
        return self._upd

    def _topology_state(self):
        """update_primitives' topology arrays, index maps and root box for the tree ``arrays`` and ``layout`` hold."""
        maps = update.index_maps(self.arrays.bvh, self.layout.prim_perm, counts_by_code(self.arrays))
        order, level_end, slot, dev = maps['order'], maps['level_end'], maps['slot_np'], self.device
        return dict(maps, order=torch.from_numpy(order).to(dev) if order.size else None,
                    slot=torch.from_numpy(slot).to(dev) if slot.size else None,
                    level_end=(C.c_int32 * max(1, level_end.size))(*level_end.tolist()), n_levels=int(level_end.size),
                    root=torch.zeros(6, dtype=torch.float32, device=dev))

    def _topology(self, st, flags):
        """The ptmi_update_topology of a call: ``flags`` None is update.refit_flags' choice for the tree's size."""
        if flags is None:
            flags = update.refit_flags(self.layout.n_inner, st['n_levels'])
        return update.UpdateTopology(st['order'].data_ptr() if st['order'] is not None else None,
                                     st['slot'].data_ptr() if st['slot'] is not None else None,
                                     st['level_end'], st['n_levels'], int(flags))

    def _pack_edits(self, edits, dtype=np.float32, stream=None):
        """``{type code: (reference indices, payload arrays...)}`` on the device, uploaded under ``stream``: one
        int32 tensor (per kind the device rows, then the leaves) and one ``dtype`` tensor (per kind its arrays in
        argument order). Returns the ``{type code: (prim ptr, leaf ptr, payload ptrs..., n)}`` the ``*_call``
        methods take, and the tensors to keep alive."""
        st = self._update_state()
        ints, payload, lists, ni, npay = [], [], {}, 0, 0
        for t, (idx, *arrays) in edits.items():
            n = idx.size
            ints += [st['dev_of'][t][idx].astype(np.int32), st['leaf_of'][t][idx].astype(np.int32)]
            starts = []
            for a in arrays:
                payload.append(a.reshape(-1))
                starts.append(npay)
                npay += a.size
            lists[t] = (ni, ni + n, *starts, n)  # element offsets, made pointers below
            ni += 2 * n
        if not ints:
            return lists, ()
        with torch.cuda.device(self.device), torch.cuda.stream(_stream_or_current(stream, self.device)):
            ti = torch.from_numpy(np.concatenate(ints)).to(self.device)  # the uploads precede the kernel on its stream
            tp = torch.from_numpy(np.concatenate(payload).astype(dtype, copy=False)).to(self.device)
        pi, pp, size = ti.data_ptr(), tp.data_ptr(), tp.element_size()  # torch allocations are 8-B aligned
        return {t: (pi + 4 * a, pi + 4 * b, *(pp + size * c for c in pay), n)
                for t, (a, b, *pay, n) in lists.items()}, (ti, tp)

    def update_call(self, lists, stream=None, flags=None):
        """ptmi_update_primitives on this scene: ``lists`` maps a primitive type
        code to (prim ptr, leaf ptr, row ptr, build ptr, count) of edits already
        on the device. ``flags``: PTMI_UPDATE_* (0: one launch per level;
        update.ONE_GROUP: the single-workgroup refit), by default
        update.refit_flags' choice for the tree's size. Asynchronous; the host
        mirror and the view are not refreshed (update_primitives does both)."""
        st, arg = self._update_state(), _list_args(update.UpdateList, lists)
        topo = self._topology(st, flags)
        with torch.cuda.device(self.device):
            _lib.check(update.load().ptmi_update_primitives(self.view, arg[0], arg[1], arg[2], C.byref(topo),
                                                            st['root'].data_ptr(), _stream_ptr(stream, self.device)),
                       'ptmi_update_primitives')

    def update_primitives(self, spheres=None, quads=None, triangles=None, stream=None, flags=None):
        """Move primitives and refit the BVH on the device (include/ptmi_update.h,
        DESIGN.md §17). Each argument is ``(reference primitive indices, rows,
        build records)``: numpy arrays of n indices, (n, 4 / 16 / 12) f32 device
        rows as include/ptmi.h lays them out and (n, 4 / 9 / 9) f32 builder-form
        records ({c, r}; {Q, u, v}; {v0, v1, v2}). Indices out of range or
        repeated, and rows that contradict their build record, are a ValueError
        before anything is uploaded. No render of this scene may be in flight
        on another stream. On return the device is updated, ``arrays`` (the
        reference-layout mirror) and ``layout`` equal what the device holds,
        the view's root box is refreshed and its shell hint re-evaluated
        (scene_data.find_shell on the mirror; 0 if the claim no longer holds).
        Topology, materials and counts do not change: materials are
        update_materials', for anything else build a new DeviceScene. ``flags``
        as for update_call (same bits either way). Tracks (set_tracks) are
        dropped if an edit names a tracked primitive: their rest rows are stale."""
        self._require_unposed()
        st = self._update_state()
        edits = update.check_edits(counts_by_code(self.layout), spheres, quads, triangles)
        if self._tracks is not None and any(np.intersect1d(idx, self._tracks['indices'].get(t, ())).size
                                            for t, (idx, _, _) in edits.items()):
            self._tracks = None
        lists, _keep = self._pack_edits(edits, stream=stream)
        self.update_call(lists, stream, flags)
        _stream_or_current(stream, self.device).synchronize()
        update.refresh_mirror(self.arrays, self.layout, st, edits,
                              self.t_ref_nodes.cpu().numpy() if self.arrays.num_bvh_nodes else None)
        self._set_tree(self.layout)

    # ------------------------------------------------ poses of moving primitives (ptmi.pose)
    def _require_unposed(self):
        if self.posed is not None:
            raise _lib.PtmiError(f'the scene is posed at t = {self.posed!r}: unpose() first')

    def set_tracks(self, spheres=None, quads=None, triangles=None, t_range=(0.0, 1.0), rigid=None):
        """Make the tracks of moving primitives resident (include/ptmi_pose.h,
        DESIGN.md §24). Each argument is ``(reference primitive indices, (n, 6 /
        9 / 12) f64 records)``: sphere {o, d}, quad {Q, d, normal}, triangle
        {v0, v1, v2, d} (``pose.track_records``); indices out of range or
        repeated and records of another shape or not finite are a ValueError.
        ``rigid``: ``(bodies, rigid.body_records(bodies, prims))``, the rigid
        bodies (include/ptmi_rigid.h) and per kind their
        ``(indices, body index per entry, (n, 3 / 15 / 18) f64 rest records)``,
        made resident next to the linear tracks; a primitive that is in a body
        and has a linear track is a ValueError. With ``rigid=None`` nothing of
        it is made and no call of it is ever issued.
        With them a *rest* edit list is uploaded: the mirror's own rows and
        build records of the tracked primitives, which ``unpose`` writes back.
        ``t_range``: the times ``pose`` will take. The shell hint of the posed
        scene is evaluated here, once: the scene is posed at both ends of the
        range, every tracked leaf gets the union of its two boxes (the box at
        any time between lies inside it: every step of the arithmetic is
        monotone in t), a leaf of a body that turns gets ``rigid.swept_box``
        instead (under rotation the two-ends argument is false), and the
        layout's hint is kept if ``find_shell`` on those boxes names the same
        leaf and that sphere is not tracked; else the posed hint is 0. The
        scene is left unposed. Replaces earlier tracks and bodies; no
        arguments clears them."""
        self._require_unposed()
        st = self._update_state()
        (t0, t1), _ = pose_mod.check_shutter(t_range, 1)
        counts = counts_by_code(self.layout)
        tracks = pose_mod.check_tracks(counts, spheres, quads, triangles)
        lists, keep = self._pack_edits(tracks, np.float64)
        indices = {t: idx for t, (idx, _) in tracks.items()}
        bodies, rigid_lists, entries, rigid_keep = [], {}, {}, ()
        if rigid is not None:
            bodies, entries = rigid_mod.check_bodies(counts, *rigid)
            for t, (idx, _, _) in entries.items():
                if np.intersect1d(idx, indices.get(t, ())).size:
                    raise ValueError('a primitive is in a rigid body and has a linear track')
            recs, rigid_keep = self._pack_edits({t: (idx, rec) for t, (idx, _, rec) in entries.items()}, np.float64)
            if entries:  # the body index of every entry, the kinds one after another as in ``recs``
                body_ids = torch.from_numpy(np.concatenate([body for _, body, _ in entries.values()])).to(self.device)
                rigid_keep += (body_ids,)
                starts = np.cumsum([0] + [body.size for _, body, _ in entries.values()])
                rigid_lists = {t: (prim, leaf, body_ids.data_ptr() + 4 * int(a), rec, n)
                               for a, (t, (prim, leaf, rec, n)) in zip(starts, recs.items())}
            indices = {t: np.union1d(indices.get(t, np.zeros(0, np.int64)), entries[t][0]) if t in entries
                       else indices[t] for t in set(indices) | set(entries)}
        rest, rest_keep = self._pack_edits(update.current_edits(self.arrays, self.layout, st, indices))
        # 'rigid_keep': the bodies' tensors, (device rows then leaves, rest records, body indices)
        self._tracks = {'lists': lists, 'rest': rest, 'keep': keep + rest_keep, 'indices': indices,
                        't_range': (t0, t1), 'shell': 0, 'bodies': bodies, 'rigid': rigid_lists,
                        'rigid_keep': rigid_keep, 'linear': bool(tracks) or not rigid_lists}
        # per type code and body that turns, the reference indices of its primitives
        self._tracks['turning'] = {(t, b): idx[body == b] for t, (idx, body, _) in entries.items()
                                   for b in np.unique(body).tolist() if bodies[b].turn != 0.0}
        self._tracks['shell'] = self._posed_shell(st, indices, t0, t1, self._tracks['turning'])

    def set_t_range(self, t_range):
        """Another ``t_range`` for the resident tracks and bodies: nothing is
        uploaded, the posed shell hint is evaluated anew (as set_tracks does).
        The per-frame step of an animation, whose shutter moves on while the
        tracks stay. Needs set_tracks() first; the scene must be unposed."""
        self._require_unposed()
        tr = self._tracks
        if tr is None:
            raise _lib.PtmiError('set_t_range needs set_tracks() first')
        tr['t_range'], _ = pose_mod.check_shutter(t_range, 1)
        tr['shell'] = 0
        tr['shell'] = self._posed_shell(self._update_state(), tr['indices'], *tr['t_range'], tr['turning'])

    def _posed_shell(self, st, indices, t0, t1, turning=None):
        """The shell hint valid at every pose in [t0, t1] (set_tracks): the layout's, or 0. ``turning``: per type
        code and body that turns, the reference indices of its primitives."""
        lay, sa = self.layout, self.arrays
        if not lay.shell or not indices:
            return int(lay.shell)
        s = torch.cuda.current_stream(self.device)
        boxes = []
        try:
            for t in (t0, t1):
                self.pose(t, s)
                boxes.append(self.t_ref_nodes.cpu().numpy().reshape(-1, 12)[:sa.num_bvh_nodes].copy())
        finally:
            self.unpose(s)
        bmin, bmax = sa.bvh['bvh_bbox_min'].copy(), sa.bvh['bvh_bbox_max'].copy()
        for t, idx in indices.items():
            leaves = st['leaf_of'][t][idx]
            bmin[leaves] = np.minimum(boxes[0][leaves, 0:3], boxes[1][leaves, 0:3])
            bmax[leaves] = np.maximum(boxes[0][leaves, 4:7], boxes[1][leaves, 4:7])
        for (t, b), idx in (turning or {}).items():  # one swept_box call per body and kind, over all its leaves
            leaves = st['leaf_of'][t][idx]
            lo, hi = rigid_mod.swept_box(sa.bvh['bvh_bbox_min'][leaves], sa.bvh['bvh_bbox_max'][leaves],
                                         self._tracks['bodies'][b], t0, t1)
            # outwards to f32: the cast alone could round a bound inwards
            bmin[leaves] = np.nextafter(lo.astype(np.float32), np.float32(-np.inf))
            bmax[leaves] = np.nextafter(hi.astype(np.float32), np.float32(np.inf))
        swept = dataclasses.replace(sa, bvh=dict(sa.bvh, bvh_bbox_min=bmin, bvh_bbox_max=bmax))
        leaf = find_shell(swept, lay.max_leaf_depth)
        if leaf <= 0 or shell_hint(swept, st['slot_np'], lay.max_leaf_depth, self._pack[0]) != lay.shell:
            return 0
        tracked = indices.get(PRIM_SPHERE)
        if tracked is not None and int(sa.bvh['bvh_prim_idx'][leaf]) in set(tracked.tolist()):
            return 0
        return int(lay.shell)

    def _pose_time(self, t):
        """The resident tracks and ``t`` as a float within their ``t_range``, or the pose calls' errors."""
        tr = self._tracks
        if tr is None:
            raise _lib.PtmiError('pose needs set_tracks() first')
        t = float(t)
        if not tr['t_range'][0] <= t <= tr['t_range'][1]:
            raise ValueError(f'pose: t = {t!r} is outside the tracks\' t_range {tr["t_range"]}')
        return tr, t

    def pose_call(self, t, stream=None, flags=None):
        """ptmi_pose_primitives on this scene's resident tracks at time ``t``:
        asynchronous; the view's host fields and ``posed`` are not touched
        (``pose`` does both). ``flags`` as for update_call."""
        tr, t = self._pose_time(t)
        st, arg = self._update_state(), _list_args(pose_mod.PoseList, tr['lists'])
        topo = self._topology(st, flags)
        with torch.cuda.device(self.device):
            _lib.check(pose_mod.load().ptmi_pose_primitives(self.view, arg[0], arg[1], arg[2], t, C.byref(topo),
                                                            st['root'].data_ptr(), _stream_ptr(stream, self.device)),
                       'ptmi_pose_primitives')
        return t

    def rigid_call(self, t, stream=None, flags=None):
        """ptmi_pose_rigid on this scene's resident bodies at time ``t``, with the
        host table ``rigid.body_table(bodies, t)``: asynchronous; the view's
        host fields and ``posed`` are not touched (``pose`` does both).
        ``flags`` as for update_call."""
        tr, t = self._pose_time(t)
        st, arg = self._update_state(), _list_args(rigid_mod.RigidList, tr['rigid'])
        topo = self._topology(st, flags)
        table = rigid_mod.body_table(tr['bodies'], t)
        with torch.cuda.device(self.device):
            _lib.check(rigid_mod.load().ptmi_pose_rigid(self.view, arg[0], arg[1], arg[2], table,
                                                        len(tr['bodies']), C.byref(topo), st['root'].data_ptr(),
                                                        _stream_ptr(stream, self.device)), 'ptmi_pose_rigid')
        return t

    def pose(self, t, stream=None, flags=None):
        """Put the tracked primitives where they are at time ``t`` and refit:
        ptmi_pose_primitives if there are linear tracks (or no bodies), then
        ptmi_pose_rigid if there are bodies. Afterwards the device holds byte
        for byte what ``update_primitives`` leaves when given
        ``pose.posed_records(tracks, t)`` and ``rigid.posed_records(bodies,
        prims, t)``. With both kinds present the tree is refitted twice per
        pose (about 40 us on the scenes measured: accepted).
        ``t`` outside set_tracks' ``t_range`` is a ValueError. One 24-byte
        readback of the root box refreshes the view; the view's shell hint
        becomes the posed one, and ``posed`` is ``t``. The mirror (``arrays``)
        and ``layout`` keep describing the rest scene; ``unpose`` brings it
        back (``pose(0.0)`` does not: Q + 0.0 * d turns a -0.0 into +0.0). No
        render of this scene may be in flight on another stream. ``flags`` as
        for update_call."""
        s = _stream_or_current(stream, self.device)
        tr, t = self._pose_time(t)
        if tr['linear']:
            self.pose_call(t, s, flags)
        if tr['rigid']:
            self.rigid_call(t, s, flags)
        self.posed = t
        if self.view.num_bvh_nodes:
            with torch.cuda.device(self.device), torch.cuda.stream(s):
                root = self._upd['root'].cpu().numpy()  # waits for the call on its stream
            self.view.root_min[:], self.view.root_max[:] = [float(x) for x in root[:3]], [float(x) for x in root[3:]]
        self.view.shell = int(self._tracks['shell'])

    def unpose(self, stream=None):
        """The rest scene back on the device: ptmi_update_primitives on the
        resident rest list restores every byte a pose changed, of linear tracks
        and of bodies; the view's root box and shell hint are the layout's
        again and ``posed`` is None. Asynchronous on ``stream``; nothing to do
        for an unposed scene."""
        if self.posed is None:
            return
        self.update_call(self._tracks['rest'], stream)
        self.posed = None
        self._set_tree(self.layout)

    # ------------------------------------------------ material edits (ptmi.material)
    def material_call(self, lists, stream=None):
        """ptmi_update_materials on this scene: ``lists`` maps a primitive type
        code to (prim ptr, leaf ptr, row ptr, count) of edits already on the
        device. Asynchronous; the host mirror and the view are not refreshed
        (update_materials does both)."""
        st, arg = self._update_state(), _list_args(material.MaterialList, lists)
        with torch.cuda.device(self.device):
            _lib.check(material.load().ptmi_update_materials(self.view, arg[0], arg[1], arg[2],
                                                             st['slot'].data_ptr() if st['slot'] is not None else None,
                                                             _stream_ptr(stream, self.device)),
                       'ptmi_update_materials')

    def update_materials(self, spheres=None, quads=None, triangles=None, stream=None):
        """Replace material rows of the resident scene on the device
        (include/ptmi_material.h). Each argument is ``(reference
        primitive indices, rows)``: numpy arrays of n indices and (n, 20) f32
        ``mats`` rows as include/ptmi.h lays them out, the flags word last.
        Indices out of range or repeated, rows of another shape or with
        non-finite values, and a flags word that names an image the scene does
        not have are a ValueError before anything is uploaded. No render of
        this scene may be in flight on another stream. On return the device is
        updated: the rows, and the material class in both copies of each edited
        primitive's leaf code. ``arrays`` (the reference-layout mirror, whose
        material arrays are the scene's own copies) and ``layout`` equal what
        the device holds: ``layout`` is pack_device of the edited arrays on the
        same BVH, byte for byte. The view's root ref is refreshed (a
        one-primitive scene's root is a leaf) and its shell hint re-evaluated:
        a shell sphere that stops being a medium clears it, an enclosing
        sphere that becomes one may gain it. Geometry, counts, topology, texels
        and the growth baseline do not change."""
        self._require_unposed()
        st = self._update_state()
        edits = material.check_edits(counts_by_code(self.layout), len(self.layout.img_w), spheres, quads, triangles)
        s = _stream_or_current(stream, self.device)
        lists, _keep = self._pack_edits(edits, stream=s)
        self.material_call(lists, s)
        s.synchronize()
        material.refresh_mirror(self.arrays, self.layout, st, edits, self._pack[0])
        self._set_tree(self.layout)

    # ------------------------------------------------ tree quality, rebuild in place (ptmi.tree)
    def _tree_state(self):
        """tree_growth's baseline areas (taken here, on the first use, and again by
        every rebuild) and its 16-byte result slot."""
        if self._tree is None:
            if self.t_ref_nodes is None:
                raise _lib.PtmiError('tree_growth needs the scene\'s ref_nodes')
            self._tree = {'base': torch.empty(max(4, self.view.num_bvh_nodes), dtype=torch.float32, device=self.device),
                          'out': torch.empty(4, dtype=torch.float32, device=self.device)}
            s = torch.cuda.current_stream(self.device)
            self._take_baseline(s)
            s.synchronize()  # an update on any stream may follow
        return self._tree

    def _take_baseline(self, stream):
        with torch.cuda.device(self.device):
            _lib.check(tree.load().ptmi_tree_areas(self.view, self._tree['base'].data_ptr(),
                                                   _stream_ptr(stream, self.device)), 'ptmi_tree_areas')

    def tree_growth(self, stream=None):
        """``(mean, max)`` over the BVH's internal nodes of box area now / box
        area when the tree was built or last rebuilt (ptmi_tree_growth,
        include/ptmi_tree.h): exactly (1.0, 1.0) on an unmoved
        or freshly rebuilt tree, growing as update_primitives scatters the
        primitives of a refit tree. One launch on ``stream`` and one 16-byte
        readback."""
        self._require_unposed()
        st = self._tree_state()
        s = _stream_or_current(stream, self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(s):
            _lib.check(tree.load().ptmi_tree_growth(self.view, st['base'].data_ptr(), st['out'].data_ptr(),
                                                    _stream_ptr(s, self.device)), 'ptmi_tree_growth')
            out = st['out'].cpu().numpy()
        return float(out[0]), float(out[1])

    def rebuild(self, stream=None, builder='host'):
        """Rebuild the BVH of the resident scene in place: the
        native SAH builder on the mirror's builder-form arrays, pack_device of
        the mirror with the new BVH, and its nodes, ref_nodes, spheres, quads,
        tris and mats copied into the tensors the scene already has. No size
        and no ``data_ptr()`` changes, so the view's pointers, an Integrator
        and every renderer built on this scene stay valid. The view's root
        ref, leaf depth, root box and shell hint are refreshed, ``layout`` and
        ``arrays.bvh`` are replaced, update_primitives' topology and index
        maps are made anew, and the growth baseline is
        retaken: tree_growth() is (1.0, 1.0) afterwards. The builder is
        deterministic, so ``layout`` equals pack_device of a compile of the
        edited world byte for byte. No render of this scene may be in flight
        (as for update_primitives); the call returns with the copies done.

        Returns a ByCode ``(spheres, triangles, quads)`` of int32 device
        tensors mapping each old device row to its new device row. Reference
        primitive indices (update_primitives' arguments) do not change; device
        rows, and so the ids of trace_guides_ids, do.

        ``builder='device'`` (include/ptmi_build.h) builds and
        packs on the device instead: the mirror's builder-form records and the
        old index maps are uploaded, ptmi_build_sah_device and ptmi_build_pack
        run on ``stream``, and the status, the seven arrays, the maps and the
        packed tensors are read back for ``arrays.bvh`` and ``layout``. What
        the device, ``layout`` and the returned maps hold is byte for byte what
        the host path leaves. A scene above ``build.MAX_PRIMS`` primitives
        (decided before any launch), a scene packed in compile order and a
        build that ends with PTMI_BUILD_NEEDS_HOST take the host path;
        ``last_rebuild`` = {'builder': 'host' | 'device', 'reason': ...} says
        which path ran and why."""
        if builder not in ('host', 'device'):
            raise ValueError(f"builder must be 'host' or 'device', not {builder!r}")
        self._require_unposed()
        self._update_state()  # the mirror (and the check that the scene was made from SceneArrays)
        s = _stream_or_current(stream, self.device)
        reason = 'asked for'
        if builder == 'device':
            maps, reason = self._rebuild_device(s)
            if maps is not None:
                self.last_rebuild = {'builder': 'device', 'reason': reason}
                return maps
        self.last_rebuild = {'builder': 'host', 'reason': reason}
        sa, old = self.arrays, self.layout
        q, t = sa.quads, sa.tris
        built = bvh_mod.build_sah(sa.sphere_data, np.concatenate([q['quad_Q'], q['quad_u'], q['quad_v']], axis=1),
                                  np.concatenate([t['triangle_v0'], t['triangle_v1'], t['triangle_v2']], axis=1))
        new_sa = dataclasses.replace(sa, bvh={k: built[k] for k in BVH_KEYS})
        lay = pack_device(new_sa, *self._pack)
        pairs = [(self.t_nodes, lay.nodes, old.nodes), (self.t_ref_nodes, lay.ref_nodes, old.ref_nodes)]
        pairs += [(getattr(self, k.tensor), getattr(lay, k.rows), getattr(old, k.rows)) for k in STORAGE]
        pairs.append((self.t_mats, lay.mats, old.mats))
        for _, a, b in pairs:
            if a.shape != b.shape:
                raise _lib.PtmiError(f'rebuild: a packed array changed its shape ({b.shape} to {a.shape})')
        with torch.cuda.device(self.device), torch.cuda.stream(s):
            for dst, a, _ in pairs:
                if a.size:
                    dst[:a.size].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
            maps = ByCode(*(torch.from_numpy(m).to(self.device)
                            for m in tree.device_maps(old.prim_perm, lay.prim_perm)))
        self._adopt_tree(lay, new_sa, s)
        return maps

    def _adopt_tree(self, lay, new_sa, s):
        """After a rebuild on either path: the new layout and mirror, the view, the update topology, the baseline."""
        self.layout, self.arrays = lay, new_sa
        self._tracks = None  # device rows, leaves and rest rows are those of the old tree
        self._set_tree(lay)
        self._upd = self._topology_state()  # leaf_of and dev_of of the new tree; the mirror is this scene's own already
        self._take_baseline(s)
        s.synchronize()

    def _rebuild_device(self, s):
        """The device path of ``rebuild``: (maps, reason), or (None, why the host path has to run)."""
        sa, old = self.arrays, self.layout
        counts = counts_by_code(old)
        n = sum(counts)
        if n > build_mod.MAX_PRIMS:
            return None, f'{n} primitives, the device builder takes {build_mod.MAX_PRIMS}'
        if n == 0 or not self._pack[1]:
            return None, 'an empty scene' if n == 0 else 'the scene is packed in compile order'
        if self._builder is None:
            self._builder = build_mod.DeviceBuilder(counts, self.device)
        b = self._builder
        sp = _stream_ptr(s, self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(s):
            b.upload(build_mod.builder_records(sa), self._upd['dev_of'])
            b.build(sp)
            b.pack(self.view, sp)
            ints, status, info, new_row, perm = b.read_ints()  # the copy waits for both kernels
            if int(status[0]) == build_mod.NEEDS_HOST:
                return None, 'PTMI_BUILD_NEEDS_HOST: a fallback segment the device does not sort'
            if int(status[0]) != 0 or int(info[10]) != 0:
                raise _lib.PtmiError(f'device rebuild: status {int(status[0])}, pack status {int(info[10])}')
            bmin, bmax = b.read_boxes()
            tensors = {'nodes': self.t_nodes, 'ref_nodes': self.t_ref_nodes, 'mats': self.t_mats}
            tensors.update({k.rows: getattr(self, k.tensor) for k in STORAGE})
            tensors = {k: t.cpu().numpy() for k, t in tensors.items()}
            a = int(b.i_off[10])
            maps = ByCode(*(b.ti[a + sum(counts[:t]):a + sum(counts[:t + 1])].clone() for t in range(3)))
        bvh = dict({k: v.copy() for k, v in ints.items()}, bvh_bbox_min=bmin.copy(), bvh_bbox_max=bmax.copy())
        new_sa = dataclasses.replace(sa, bvh={k: bvh[k] for k in BVH_KEYS})
        slot, _ = node_slots(bvh['bvh_left_child'], bvh['bvh_right_child'], bvh['bvh_prim_idx'] >= 0)
        shell = shell_hint(new_sa, slot, int(info[1]), self._pack[0])
        lay = build_mod.layout_of(old, tensors, info, perm, shell)
        self._adopt_tree(lay, new_sa, s)
        return maps, 'asked for'

    def remap_ids(self, ids, maps, out=None, stream=None):
        """An id image (trace_guides_ids) of this scene before a rebuild carried
        to the device rows after it (ptmi_ids_remap, include/ptmi_tree.h):
        ``maps`` is rebuild()'s return value; an id whose type, row or map entry
        is out of range becomes -1. Returns a new tensor, or ``out`` (which may
        be ``ids`` itself). Asynchronous on ``stream``."""
        _check_tensor('ids', ids, ('H', 'W'), torch.int32, self.device)
        counts = counts_by_code(self.layout)
        maps = tuple(maps)
        if len(maps) != 3:
            raise _lib.PtmiError(f'maps must be ({", ".join(ByCode._fields)})')
        for m, n, name in zip(maps, counts, ByCode._fields):
            _check_tensor(f'maps: {name}', m, (n,), torch.int32, self.device)
        with torch.cuda.device(self.device):
            if out is None:
                with torch.cuda.stream(_stream_or_current(stream, self.device)):
                    out = torch.empty_like(ids)
            _check_tensor('out', out, tuple(ids.shape), torch.int32, self.device)
            ptr = [m.data_ptr() if n else None for m, n in zip(maps, counts)]
            _lib.check(tree.load().ptmi_ids_remap(ids.data_ptr(), out.data_ptr(), ids.numel(), ptr[0], ptr[1], ptr[2],
                                                  tree.IdsCounts(*counts), _stream_ptr(stream, self.device)),
                       'ptmi_ids_remap')
        return out

    def permute_rows(self, rows, maps, stream=None):
        """``primitive_rows()`` taken before a rebuild, in the device order after
        it, both ByStorage: row ``maps[t][k]`` of the result is row k of
        ``rows``. ``maps`` is rebuild()'s ByCode."""
        out = []
        with torch.cuda.device(self.device), torch.cuda.stream(_stream_or_current(stream, self.device)):
            for k, r in zip(STORAGE, rows):
                n, w, new = getattr(self.layout, k.count), k.row_floats, r.clone()
                if n:
                    new[:n * w].view(n, w)[maps[k.code].long()] = r[:n * w].view(n, w)
                out.append(new)
        return ByStorage(*out)


def make_frame(cam, bg, max_depth, seed, width, height, window=None, band=(1, 1, 0), traversal='stack'):
    """ptmi_frame from camera upload values (dict of f32 3-vectors or an
    object with the reference camera's attributes). ``traversal``: 'stack'
    (traverse_bvh_legacy, the reference's default) or 'stackless'
    (traverse_bvh_stackless, its USE_STACKLESS_TRAVERSAL = True)."""
    f = _lib.Frame()
    if traversal not in _lib.TRAVERSALS:
        raise _lib.PtmiError(f'unknown traversal {traversal!r} (one of {sorted(_lib.TRAVERSALS)})')
    f.traversal = _lib.TRAVERSALS[traversal]
    vals = cam if isinstance(cam, dict) else camera_upload(cam)
    get = vals.__getitem__
    for k, fld in (('center', 'center'), ('pixel00', 'pixel00'), ('delta_u', 'delta_u'), ('delta_v', 'delta_v'),
                   ('defocus_u', 'defocus_u'), ('defocus_v', 'defocus_v')):
        arr = np.asarray(get(k), np.float32)
        for i in range(3):
            getattr(f.cam, fld)[i] = float(arr[i])
    f.cam.defocus_angle = float(np.float32(get('defocus_angle')))
    bgv = np.asarray([bg.x, bg.y, bg.z] if hasattr(bg, 'x') else bg, np.float64).astype(np.float32)
    for i in range(3):
        f.bg[i] = float(bgv[i])
    f.max_depth = int(max_depth)
    f.seed = int(seed) & 0xffffffff
    f.width, f.height = int(width), int(height)
    x0, y0, w, h = window if window is not None else (0, 0, width, height)
    f.x0, f.y0, f.w, f.h = int(x0), int(y0), int(w), int(h)
    f.band_rows, f.band_stride, f.band_offset = (int(b) for b in band)
    return f


def frame_pixel_rows(frame):
    """Image rows owned by a frame (window + band filter), as the kernels see them."""
    rows = [frame.y0 + r for r in range(frame.h)
            if (r // frame.band_rows) % frame.band_stride == frame.band_offset]
    return np.asarray(rows, np.int64)


class Integrator:
    """Launch wrapper: megakernel / wavefront / clear / tonemap on one stream."""

    def __init__(self, dscene: DeviceScene, with_counters=True):
        self.scene = dscene
        self.lib = _lib.load()
        self.counters = torch.zeros(_lib.NUM_COUNTERS, dtype=torch.int64, device=dscene.device) \
            if with_counters else None
        self._ws = None
        self._ws_bytes = 0
        self._reset_event = None  # counter reset the next overlapped trace must wait for
        self._ov = None  # side streams, workspaces and events of render_mk_overlapped, made by its first call
        self._n_active = torch.zeros(1, dtype=torch.int32, device=dscene.device)  # tile_update's readback slot
        self._dn_ws = None  # denoise's two working images, made by its first call

    def _call(self, name, *args):
        """One C-ABI call by export name; a non-zero return raises PtmiError with ptmi_last_error()."""
        return _lib.check(getattr(self.lib, name)(*args), name)

    def _batch(self, frame, npix, sample_count, one_trace=False):
        """Samples per batch of a call on the frame's npix pixels: all of them,
        within the staging budget (12 B per sample and pixel) and, where a
        batch is one trace (one_trace), within its 32-bit item ids
        (ptmi_mk_max_batch)."""
        n = min(int(sample_count), self.STAGING_BYTES // max(1, 12 * npix))
        if one_trace:
            max_batch = int(self.lib.ptmi_mk_max_batch(frame))
            if max_batch < 1:
                _lib.check(-1, 'ptmi_mk_max_batch')
            n = min(n, max_batch)
        return max(1, n)

    def _cnt(self):
        return self.counters.data_ptr() if self.counters is not None else None

    def _dev(self):
        """Context that makes the scene's device current for a C-ABI call."""
        return torch.cuda.device(self.scene.device)

    def _stream(self, stream):
        return _stream_ptr(stream, self.scene.device)

    # the per-pixel buffers the host layer takes: the shape after (height, width), and the dtype
    IMAGE_KINDS = {'accum': ((3,), torch.float32), 'stats': ((4,), torch.float32), 'out': ((3,), torch.float32),
                   'guides': ((guide.GUIDE_CHANNELS,), torch.float32), 'ids': ((), torch.int32),
                   'var': ((), torch.float32)}

    def _check_image(self, kind, t, height, width):
        """``t`` is a ``kind`` buffer of a height x width image on the scene's device (_check_tensor)."""
        tail, dtype = self.IMAGE_KINDS[kind]
        _check_tensor(kind, t, (height, width) + tail, dtype, self.scene.device)

    # multi-sample megakernel calls run as (tile, sample chunk) work units with
    # staged colours (ptmi_mk_render_ws); single samples accumulate directly
    MK_STAGED_MIN_SAMPLES = 2

    def render_mk(self, frame, accum, sample_begin, sample_count, stream=None, staged=None, overlap=False):
        """Megakernel render of samples [sample_begin, sample_begin + sample_count)
        added into accum in sample order. overlap=True: consecutive calls
        pipeline (see render_mk_overlapped)."""
        self._check_image('accum', accum, frame.height, frame.width)
        if overlap:
            return self.render_mk_overlapped(frame, accum, sample_begin, sample_count, stream)
        if staged is None:
            staged = int(sample_count) >= self.MK_STAGED_MIN_SAMPLES
        with self._dev():
            if staged:
                ws = self.workspace(frame, sample_count, 'mk')
                self._call('ptmi_mk_render_ws', self.scene.view, frame, ws.data_ptr(), self._ws_bytes,
                           accum.data_ptr(), int(sample_begin), int(sample_count), self._cnt(), self._stream(stream))
                return
            self._call('ptmi_mk_render', self.scene.view, frame, accum.data_ptr(), int(sample_begin),
                       int(sample_count), self._cnt(), self._stream(stream))

    # Staging budget for the per-(sample, pixel) colour slots of one batch:
    # 2 GiB keeps a whole 16-spp 4K call (1.6 GB) in one batch. A/B on MI355X
    # (PTMI_STAGING_BYTES, A/B only): C5 3757 (1 GiB: 10 + 6 spp batches) ->
    # 3788 Msamples/s, C2 unchanged, 4 GiB no further change
    # (profiles/r03/ab/ab_staging_bytes.log).
    STAGING_BYTES = int(os.environ.get('PTMI_STAGING_BYTES', str(2 << 30)))
    # Overlapped megakernel calls: traces in flight, one workspace and side
    # stream each. Round 3 measured two in flight for whole-frame calls and
    # three for small calls (vol2 800x800, 64 spp per call: the full frame,
    # 41 M samples per call, 2851 (2) vs 2762 (3) Msamples/s; an 8-GPU tile
    # shard, 5.1 M samples per call, 2380-2487 (2) vs 2450-2565 (3); 4 slower
    # than both; profiles/r03/overlap_depth_and_bands.log). Since draining
    # waves traverse at the lowest priority (pt_megakernel.hip,
    # PTMI_MK_PRIO_DRAIN) three are as fast on whole frames too: C2 3314 vs
    # 3312, C5 4306 vs 4314, C4 1786 vs 1760; the shard 3085 (3) vs 2985 (2)
    # vs 3092 (4) (profiles/r05/overlap_depth_r05.log), so three always.
    # PTMI_OVERLAP_DEPTH fixes the depth (A/B only).
    OVERLAP_DEPTH_MAX = 3

    def render_mk_overlapped(self, frame, accum, sample_begin, sample_count, stream=None):
        """Megakernel calls whose launches overlap: each batch is traced
        (ptmi_mk_trace_ws) on one of two side streams into one of two
        workspaces, alternately, and resolved (ptmi_mk_resolve_ws) on the
        caller's stream in call order, so the next call's megakernel fills
        the chip while the previous one's last long paths drain (~1.5 ms of a
        17-ms vol2 launch otherwise leaves most of the chip idle). Results
        are bit-identical to render_mk: the resolves add the same staged
        colours in the same sample order.

        Ordering, whatever stream each call passes:
        * a trace into workspace half h waits for the resolve that last read
          half h (an event recorded on the stream that ran that resolve), and
          for every counter reset issued before it (reset_counters makes
          every side stream wait on its event; the reset and read_counters in
          turn wait for the traces still adding to the counters, whatever
          stream they run on);
        * a resolve waits for its own trace and for the previous resolve, so
          the accumulator sees the batches in call order;
        * a trace does not wait for other work the caller queued after the
          previous call: the scene must not change between overlapped calls,
          and work on the caller's stream after this call sees the resolved
          accumulator as usual."""
        dev = self.scene.device
        caller = _stream_or_current(stream, dev)
        npix = frame.w * len(frame_pixel_rows(frame))
        if npix == 0 or sample_count <= 0:
            return
        per = self._batch(frame, npix, sample_count, one_trace=True)
        with self._dev():
            if self._ov is None:
                D = self.OVERLAP_DEPTH_MAX
                self._ov = {'streams': [torch.cuda.Stream(dev) for _ in range(D)], 'ws': [None] * D,
                            'k': 0, 'resolved': [None] * D, 'last_resolved': None, 'traced': [None] * D}
                if self._reset_event is not None:  # a reset issued before the side streams existed
                    for side in self._ov['streams']:
                        side.wait_event(self._reset_event)
            ov = self._ov
            depth = int(os.environ.get('PTMI_OVERLAP_DEPTH', '0')) or self.OVERLAP_DEPTH_MAX
            depth = max(1, min(depth, len(ov['ws'])))
            b = 0
            while b < sample_count:
                n = min(per, int(sample_count) - b)
                h = ov['k'] % depth  # any rotation is safe: each half waits for its own last reader
                ov['k'] += 1
                need = int(self.lib.ptmi_mk_workspace_bytes(frame, n))
                if need == 0:
                    _lib.check(-1, 'ptmi_mk_workspace_bytes')
                side = ov['streams'][h]
                ws = ov['ws'][h]
                if ws is None or ws.numel() * 4 < need:
                    torch.cuda.synchronize(dev)  # the old half may still be read by a trace or a resolve
                    ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)
                    ov['ws'][h] = ws
                    fresh = torch.cuda.Event()
                    fresh.record(torch.cuda.current_stream(dev))  # the allocation's stream
                    side.wait_event(fresh)
                if ov['resolved'][h] is not None:
                    side.wait_event(ov['resolved'][h])
                self._call('ptmi_mk_trace_ws', self.scene.view, frame, ws.data_ptr(), ws.numel() * 4,
                           int(sample_begin) + b, n, self._cnt(), side.cuda_stream)
                traced = torch.cuda.Event()
                traced.record(side)
                ov['traced'][h] = traced
                caller.wait_event(traced)
                if ov['last_resolved'] is not None:
                    caller.wait_event(ov['last_resolved'])
                self._call('ptmi_mk_resolve_ws', frame, ws.data_ptr(), ws.numel() * 4, accum.data_ptr(), n,
                           caller.cuda_stream)
                done = torch.cuda.Event()
                done.record(caller)
                ov['resolved'][h] = done
                ov['last_resolved'] = done
                b += n

    def workspace(self, frame, sample_count=1, kind='wf'):
        """Cached device workspace (torch) big enough for one batch of the call
        (shared by the megakernel's staged mode and the wavefront)."""
        fn = self.lib.ptmi_wf_workspace_bytes if kind == 'wf' else self.lib.ptmi_mk_workspace_bytes
        npix = frame.w * len(frame_pixel_rows(frame))
        need = int(fn(frame, self._batch(frame, npix, sample_count)))
        if need == 0:
            _lib.check(-1, f'ptmi_{kind}_workspace_bytes')
        if self._ws is None or self._ws_bytes < need:
            self._ws = None
            self._ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=self.scene.device)
            self._ws_bytes = self._ws.numel() * 4
        return self._ws

    def render_wf(self, frame, accum, sample_begin, sample_count, stream=None):
        self._check_image('accum', accum, frame.height, frame.width)
        with self._dev():
            ws = self.workspace(frame, sample_count)
            self._call('ptmi_wf_render', self.scene.view, frame, ws.data_ptr(), self._ws_bytes, accum.data_ptr(),
                       int(sample_begin), int(sample_count), self._cnt(), self._stream(stream))

    def clear(self, frame, accum, stream=None):
        self._check_image('accum', accum, frame.height, frame.width)
        with self._dev():
            self._call('ptmi_clear', frame, accum.data_ptr(), self._stream(stream))

    def tonemap(self, accum, spp=None, stats=None, stream=None):
        """u8 image of accum divided by ``spp``, or, with ``stats``, by each
        pixel's own sample count (ptmi_tonemap_stats)."""
        if accum.device != self.scene.device:
            raise _lib.PtmiError(f'accum is on {accum.device}, the scene on {self.scene.device}')
        if (spp is None) == (stats is None):
            raise _lib.PtmiError('tonemap needs exactly one of spp and stats')
        h, w, _ = accum.shape
        with self._dev():
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=accum.device)
            if stats is not None:
                self._check_image('stats', stats, h, w)
                self._call('ptmi_tonemap_stats', accum.data_ptr(), stats.data_ptr(), out.data_ptr(), w, h,
                           self._stream(stream))
                return out
            self._call('ptmi_tonemap', accum.data_ptr(), out.data_ptr(), w, h, int(spp), self._stream(stream))
        return out

    # ------------------------------------------ error estimates, adaptive tiles
    def tile_grid(self, frame):
        """(tile_w, tile_h, tiles_x, tiles_y) of the frame's 64-pixel megakernel tiles."""
        v = [C.c_int32() for _ in range(4)]
        self._call('ptmi_mk_tile_grid', frame, *v)
        return tuple(int(x.value) for x in v)

    def new_stats(self, frame):
        """A zeroed stats buffer ({n, mean, M2, 0} per pixel) for the frame's image."""
        return torch.zeros((frame.height, frame.width, 4), dtype=torch.float32, device=self.scene.device)

    def new_tiles(self, frame):
        """Tile buffers of a frame: state (all active), error, active list and its length."""
        _, _, tx, ty = self.tile_grid(frame)
        dev = self.scene.device
        return {'state': torch.ones(tx * ty, dtype=torch.int32, device=dev),
                'err': torch.full((tx * ty,), float('inf'), dtype=torch.float32, device=dev),
                'list': torch.arange(tx * ty, dtype=torch.int32, device=dev), 'n': tx * ty, 'grid': (tx, ty)}

    def clear_stats(self, frame, stats, stream=None):
        self._check_image('stats', stats, frame.height, frame.width)
        with self._dev():
            self._call('ptmi_stats_clear', frame, stats.data_ptr(), self._stream(stream))

    def render_mk_stats(self, frame, accum, stats, sample_begin, sample_count, tiles=None, stream=None):
        """Megakernel samples [sample_begin, sample_begin + sample_count) added
        into accum in sample order and into stats (Welford on the luminance):
        always the staged trace plus the stats resolve, single samples
        included. ``tiles``: None for the whole frame, or (int32 device tensor
        of tile ids, count): only those tiles are traced and resolved."""
        self._check_image('accum', accum, frame.height, frame.width)
        self._check_image('stats', stats, frame.height, frame.width)
        sample_count = int(sample_count)
        tl, nt = _check_tiles(tiles, self.scene.device)
        npix = frame.w * len(frame_pixel_rows(frame))
        if npix == 0 or sample_count <= 0 or (tl is not None and nt == 0):
            return
        per = self._batch(frame, npix, sample_count, one_trace=True)
        with self._dev():
            ws = self.workspace(frame, per, 'mk')
            wp, sp = ws.data_ptr(), self._stream(stream)
            tp = tl.data_ptr() if tl is not None else None
            for b in range(0, sample_count, per):
                n = min(per, sample_count - b)
                if tl is None:
                    self._call('ptmi_mk_trace_ws', self.scene.view, frame, wp, self._ws_bytes, int(sample_begin) + b,
                               n, self._cnt(), sp)
                else:
                    self._call('ptmi_mk_trace_tiles_ws', self.scene.view, frame, wp, self._ws_bytes, tp, nt,
                               int(sample_begin) + b, n, self._cnt(), sp)
                self._call('ptmi_mk_resolve_stats_ws', frame, wp, self._ws_bytes, accum.data_ptr(), stats.data_ptr(),
                           tp, nt, n, sp)

    def render_wf_stats(self, frame, accum, stats, sample_begin, sample_count, tiles=None, stream=None):
        """render_wf resolving through the stats resolve. ``tiles``: None for
        the whole frame, or (int32 device tensor of tile ids, count): only
        those tiles are traced and resolved (ptmi_wf_render_tiles_stats,
        include/ptmi_wf_tiles.h); an empty list returns at once."""
        self._check_image('accum', accum, frame.height, frame.width)
        self._check_image('stats', stats, frame.height, frame.width)
        tl, nt = _check_tiles(tiles, self.scene.device)
        if tl is not None and nt == 0:
            return
        with self._dev():
            ws = self.workspace(frame, sample_count)
            if tl is not None:
                _lib.check(wf_tiles.load().ptmi_wf_render_tiles_stats(
                    self.scene.view, frame, ws.data_ptr(), self._ws_bytes, accum.data_ptr(), stats.data_ptr(),
                    tl.data_ptr(), nt, int(sample_begin), int(sample_count), self._cnt(), self._stream(stream)),
                    'ptmi_wf_render_tiles_stats')
                return
            self._call('ptmi_wf_render_stats', self.scene.view, frame, ws.data_ptr(), self._ws_bytes,
                       accum.data_ptr(), stats.data_ptr(), int(sample_begin), int(sample_count), self._cnt(),
                       self._stream(stream))

    def tile_update(self, frame, stats, threshold, min_spp, max_spp, tiles, stream=None):
        """Tile errors and states from stats (ptmi_tile_update) into the
        buffers of ``tiles`` (new_tiles); returns the number of active tiles
        (one 4-byte readback) and stores it as tiles['n']."""
        self._check_image('stats', stats, frame.height, frame.width)
        with self._dev():
            self._call('ptmi_tile_update', frame, stats.data_ptr(), float(threshold), int(min_spp), int(max_spp),
                       tiles['state'].data_ptr(), tiles['err'].data_ptr(), tiles['list'].data_ptr(),
                       self._n_active.data_ptr(), self._stream(stream))
            if stream is not None:
                stream.synchronize()
            tiles['n'] = int(self._n_active.item())
        return tiles['n']

    # ------------------------------------------------ post-processing (ptmi.post)
    def _check_denoise_inputs(self, accum, stats):
        """(height, width) of an (accum, stats) pair of one image, of any size."""
        _check_tensor('accum', accum, ('H', 'W', 3), torch.float32, self.scene.device)
        h, w = int(accum.shape[0]), int(accum.shape[1])
        self._check_image('stats', stats, h, w)
        return h, w

    def _denoise_buffers(self, h, w, out, var):
        """The outputs (made if not given) and the cached workspace of a denoise call."""
        dev = self.scene.device
        need = post.workspace_bytes(w, h)
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        if var is None:
            var = torch.empty((h, w), dtype=torch.float32, device=dev)
        self._check_image('out', out, h, w)
        self._check_image('var', var, h, w)
        if self._dn_ws is None or self._dn_ws.numel() * 4 < need:
            self._dn_ws = None
            self._dn_ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
        return out, var, self._dn_ws

    def denoise(self, accum, stats, iterations=5, sigma=4.0, out=None, var=None, stream=None):
        """Variance-guided a-trous filter of accum by the error estimates in
        stats (ptmi_denoise, include/ptmi_post.h), asynchronous on ``stream``.
        Returns (rgb (H, W, 3) f32, var (H, W) f32: the variance the filter
        claims for the result); ``out`` and ``var`` are used if given. The
        workspace is cached on the integrator."""
        lib = post.load()
        h, w = self._check_denoise_inputs(accum, stats)
        with self._dev():
            out, var, ws = self._denoise_buffers(h, w, out, var)
            _lib.check(lib.ptmi_denoise(accum.data_ptr(), stats.data_ptr(), w, h, int(iterations), float(sigma),
                                        ws.data_ptr(), ws.numel() * 4, out.data_ptr(),
                                        var.data_ptr(), self._stream(stream)), 'ptmi_denoise')
        return out, var

    # ------------------------------------------------ guides (ptmi.guide, ptmi.motion)
    def trace_guides(self, frame, out=None, stream=None):
        """First-hit guide buffers of a whole, unbanded frame (ptmi_guide_trace,
        include/ptmi_guide.h): an (H, W, 8) f32 tensor {nx, ny, nz, depth, ar,
        ag, ab, hit} from one deterministic primary ray per pixel,
        asynchronous on ``stream``; ``out`` is used if given."""
        return self._trace_guides(frame, out, stream, False)[0]

    def trace_guides_ids(self, frame, out=None, stream=None):
        """``trace_guides`` that also returns which primitive each pixel sees
        (ptmi_guide_trace_ids, include/ptmi_motion.h): ``(guides, ids)``, the
        guides byte for byte ``trace_guides``', ids an (H, W) int32 tensor of
        ``type << 28 | device primitive index`` on surface hits and -1
        elsewhere. ``out``: a (guides, ids) pair to write into."""
        return self._trace_guides(frame, out, stream, True)

    def _trace_guides(self, frame, out, stream, with_ids):
        """trace_guides and trace_guides_ids: ptmi_guide_trace, or with the id image ptmi_guide_trace_ids."""
        lib = (motion if with_ids else guide).load()
        dev = self.scene.device
        h, w = int(frame.height), int(frame.width)
        with self._dev():
            if out is None:
                out = (torch.empty((h, w, guide.GUIDE_CHANNELS), dtype=torch.float32, device=dev),
                       torch.empty((h, w), dtype=torch.int32, device=dev) if with_ids else None)
            elif not with_ids:
                out = (out, None)
            guides, ids = out
            self._check_image('guides', guides, h, w)
            if with_ids:
                self._check_image('ids', ids, h, w)
                _lib.check(lib.ptmi_guide_trace_ids(self.scene.view, frame, guides.data_ptr(), ids.data_ptr(),
                                                    self._stream(stream)), 'ptmi_guide_trace_ids')
            else:
                _lib.check(lib.ptmi_guide_trace(self.scene.view, frame, guides.data_ptr(), self._stream(stream)),
                           'ptmi_guide_trace')
        return guides, ids

    def denoise_guided(self, accum, stats, guides, iterations=5, sigma=4.0, sigma_z=0.1, sigma_a=0.2,
                       normal_power_log2=5, demodulate=True, out=None, var=None, stream=None):
        """``denoise`` with the guides of ``trace_guides`` as further
        edge-stopping terms (relative depth, albedo, normal) and, with
        ``demodulate``, the filter run on colour divided by the albedo
        (ptmi_denoise_guided, include/ptmi_guide.h). Same return values and
        the same cached workspace as ``denoise``."""
        lib = guide.load()
        h, w = self._check_denoise_inputs(accum, stats)
        self._check_image('guides', guides, h, w)
        prm = guide.params(iterations, sigma, sigma_z, sigma_a, normal_power_log2, demodulate)
        with self._dev():
            out, var, ws = self._denoise_buffers(h, w, out, var)
            _lib.check(lib.ptmi_denoise_guided(accum.data_ptr(), stats.data_ptr(), guides.data_ptr(), w, h,
                                               C.byref(prm), ws.data_ptr(), ws.numel() * 4, out.data_ptr(),
                                               var.data_ptr(), self._stream(stream)), 'ptmi_denoise_guided')
        return out, var

    # ------------------------------------ temporal reprojection (ptmi.temporal, ptmi.motion)
    def reproject(self, cur_cam, prev_cam, guides_cur, guides_prev, accum, stats, *, max_history=32.0, sigma_z=0.1,
                  normal_min=0.9, sigma_a=0.2, out=None, stream=None):
        """The history ``accum``, ``stats`` of a stats render from ``prev_cam``
        carried to ``cur_cam`` (ptmi_reproject, include/ptmi_temporal.h): every
        pixel of the current frame finds its surface point in the previous
        frame, checks by both guide images (``trace_guides`` of each camera)
        that it is the same surface, and takes colour, per-sample luminance
        variance and a sample count capped at ``max_history`` from there;
        pixels without history are zero. The cameras are camera-upload dicts
        or ``_lib.Camera`` values. Returns (accum, stats) as new tensors, or
        the pair ``out`` if given; asynchronous on ``stream``."""
        return self._reproject(cur_cam, prev_cam, guides_cur, guides_prev, accum, stats,
                               (max_history, sigma_z, normal_min, sigma_a), out, stream)

    def reproject_moved(self, cur_cam, prev_cam, guides_cur, guides_prev, ids_cur, ids_prev, prev_rows, accum, stats, *,
                        max_history=32.0, sigma_z=0.1, normal_min=0.9, sigma_a=0.2, match_ids=True, out=None,
                        stream=None):
        """``reproject`` across a scene update (ptmi_reproject_moved,
        include/ptmi_motion.h): a hit pixel's surface point is first carried to
        where it was on its primitive before the update, by the primitive's
        current row (this scene's) and its previous row (``prev_rows``, the
        ``DeviceScene.primitive_rows()`` taken before the update); with
        ``match_ids`` a tap must also show the same primitive. ``ids_cur`` and
        ``ids_prev`` are ``trace_guides_ids``' id images of the two frames.
        Everything else, the return value included, is ``reproject``'s."""
        return self._reproject(cur_cam, prev_cam, guides_cur, guides_prev, accum, stats,
                               (max_history, sigma_z, normal_min, sigma_a), out, stream,
                               (ids_cur, ids_prev, prev_rows, match_ids))

    def _reproject(self, cur_cam, prev_cam, guides_cur, guides_prev, accum, stats, prm, out, stream, moved=None):
        """reproject, or with ``moved`` = (ids_cur, ids_prev, prev_rows, match_ids) reproject_moved:
        ptmi_reproject or ptmi_reproject_moved. ``prm``: (max_history, sigma_z, normal_min, sigma_a)."""
        lib = (motion if moved else temporal).load()
        h, w = self._check_denoise_inputs(accum, stats)
        self._check_image('guides', guides_cur, h, w)
        self._check_image('guides', guides_prev, h, w)
        if moved:
            ids_cur, ids_prev, prev_rows, match_ids = moved
            self._check_image('ids', ids_cur, h, w)
            self._check_image('ids', ids_prev, h, w)
            rows = tuple(prev_rows)
            if len(rows) != 3:
                raise _lib.PtmiError(f'prev_rows must be ({", ".join(ByStorage._fields)})')
            for t, k, name in zip(rows, STORAGE, ByStorage._fields):
                _check_tensor(f'prev_rows: {name}', t, tuple(getattr(self.scene, k.tensor).shape), torch.float32,
                              self.scene.device)
        cur, prev = temporal.camera(cur_cam), temporal.camera(prev_cam)
        prm = motion.params(*prm, match_ids) if moved else temporal.params(*prm)
        with self._dev():
            if out is None:
                out = (torch.empty_like(accum), torch.empty_like(stats))
            out_accum, out_stats = out
            self._check_denoise_inputs(out_accum, out_stats)
            if tuple(out_accum.shape) != tuple(accum.shape):
                raise _lib.PtmiError(f'out must be an (accum, stats) pair of a {w} x {h} image')
            head = (C.byref(cur), C.byref(prev), guides_cur.data_ptr(), guides_prev.data_ptr(), accum.data_ptr(),
                    stats.data_ptr())
            tail = (w, h, C.byref(prm), out_accum.data_ptr(), out_stats.data_ptr(), self._stream(stream))
            if moved:
                _lib.check(lib.ptmi_reproject_moved(*head, ids_cur.data_ptr(), ids_prev.data_ptr(), self.scene.view,
                                                    *(r.data_ptr() for r in rows), *tail),
                           'ptmi_reproject_moved')
            else:
                _lib.check(lib.ptmi_reproject(*head, *tail), 'ptmi_reproject')
        return out_accum, out_stats

    # ------------------------------------------------ history validation (ptmi.validate)
    def validate_history(self, hist_accum, hist_stats, fresh_accum, fresh_stats, *, radius=3, k_lo=2.0, k_hi=4.0,
                         out=None, weight=None, stream=None):
        """A carried history (``reproject``'s or ``reproject_moved``'s output)
        validated against a stats render of the current scene from cleared
        buffers and merged with it (ptmi_history_validate,
        include/ptmi_validate.h): over a window of ``(2 radius + 1)^2`` pixels
        the difference of the two mean luminances is set against its own
        standard error; up to ``k_lo`` standard errors the history of the
        window's pixel is kept, from ``k_hi`` on it is dropped, in between in
        proportion. Returns (accum, stats) as new tensors, or the pair ``out``
        if given (not one of the inputs); ``weight``, an (H, W) f32 tensor, if
        given receives the kept fraction n_v / n_h of every pixel.
        Asynchronous on ``stream``."""
        lib = validate.load()
        h, w = self._check_denoise_inputs(hist_accum, hist_stats)
        self._check_image('accum', fresh_accum, h, w)
        self._check_image('stats', fresh_stats, h, w)
        prm = validate.params(radius, k_lo, k_hi)
        with self._dev():
            if out is None:
                out = (torch.empty_like(hist_accum), torch.empty_like(hist_stats))
            out_accum, out_stats = out
            self._check_image('accum', out_accum, h, w)
            self._check_image('stats', out_stats, h, w)
            if weight is not None:
                self._check_image('var', weight, h, w)
            _lib.check(lib.ptmi_history_validate(hist_accum.data_ptr(), hist_stats.data_ptr(), fresh_accum.data_ptr(),
                                                 fresh_stats.data_ptr(), w, h, C.byref(prm), out_accum.data_ptr(),
                                                 out_stats.data_ptr(),
                                                 weight.data_ptr() if weight is not None else None,
                                                 self._stream(stream)), 'ptmi_history_validate')
        return out_accum, out_stats

    # ------------------------------------------------ motion blur by poses (ptmi.pose)
    def render_posed(self, render_fn, frame, sample_begin, sample_count, slice_spp, shutter, *args, stream=None,
                     **kwargs):
        """Samples [sample_begin, sample_begin + sample_count) rendered as a
        sequence of poses of the scene's tracks (DeviceScene.set_tracks,
        DESIGN.md §24): the range is split on the global slice boundaries
        (``pose.slice_times``: sample s belongs to slice s // slice_spp, however
        the render is chunked), and for every slice the scene is posed at the
        slice's shutter time and ``render_fn(frame, *args, begin, count,
        **kwargs)`` renders the overlap: ``render_mk`` with ``args = (accum,)``,
        ``render_mk_stats`` with ``(accum, stats)`` and ``tiles=``. A pose
        writes the scene, so its stream first waits for every overlapped trace
        in flight: overlapped megakernel calls never straddle a pose, within a
        slice they stay overlapped; the pose's own root readback has finished
        it before the slice's first trace is launched on any stream. The scene
        is left posed: the caller unposes (``unpose``)."""
        dev = self.scene.device
        s = _stream_or_current(stream, dev)
        if stream is not None:
            kwargs['stream'] = stream
        for _, t, begin, n in pose_mod.slice_times(sample_begin, sample_count, slice_spp, shutter):
            self._after_traces(s)
            self.scene.pose(t, s)
            render_fn(frame, *args, begin, n, **kwargs)

    def unpose(self, stream=None):
        """The scene's rest state back (DeviceScene.unpose), after every overlapped trace in flight."""
        s = _stream_or_current(stream, self.scene.device)
        self._after_traces(s)
        self.scene.unpose(s)

    def _after_traces(self, stream):
        """Make `stream` wait for the overlapped traces in flight: they add to
        the counters from their side streams."""
        if self._ov is not None:
            for ev in self._ov['traced']:
                if ev is not None:
                    stream.wait_event(ev)

    def read_counters(self):
        if self.counters is None:
            return None
        self._after_traces(torch.cuda.current_stream(self.scene.device))
        c = self.counters.cpu().numpy()
        return {'segments': int(c[0]), 'medium': int(c[1]), 'paths': int(c[2]), 'rr': int(c[3]),
                'depth_cap': int(c[4])}

    def tail_segments(self):
        """Segments the wavefront traced in its one-launch tail (wf_drain):
        part of read_counters()['segments'], counted apart so per-kernel
        rates attribute them to the launch that traced them."""
        if self.counters is None:
            return None
        self._after_traces(torch.cuda.current_stream(self.scene.device))
        return int(self.counters[_lib.COUNTER_TAIL_SEGMENTS].item())

    def reset_counters(self, stream=None):
        if self.counters is not None:
            s = _stream_or_current(stream, self.scene.device)
            self._after_traces(s)
            with torch.cuda.stream(s):
                self.counters.zero_()
            # overlapped traces run on side streams: every later trace, on any of
            # them, waits for this reset (a multi-batch call rotates through the
            # side streams, so waiting on the first one only is not enough)
            ev = torch.cuda.Event()
            ev.record(s)
            if self._ov is not None:
                for side in self._ov['streams']:
                    side.wait_event(ev)
            self._reset_event = ev  # side streams created after this reset wait on it too


def _check_tensor(name, t, shape, dtype, device):
    """The host layer's one argument check: ``t`` is a contiguous cuda tensor of
    ``dtype`` and ``shape`` on ``device``. A str in ``shape`` stands for any
    size and names it in the message. Raises PtmiError."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
            and t.dim() == len(shape) and all(isinstance(n, str) or n == m for n, m in zip(shape, t.shape))):
        raise _lib.PtmiError(f'{name} must be a contiguous cuda {str(dtype).split(".")[-1]} tensor of shape '
                             f'({", ".join(str(n) for n in shape)})')
    if t.device != device:
        raise _lib.PtmiError(f'{name} is on {t.device}, the scene on {device}')


def _check_tiles(tiles, device):
    """(tensor or None, count) of a ``tiles`` argument: None, or (int32 tensor of tile ids on ``device``, count)."""
    tl, nt = (None, 0) if tiles is None else tiles
    if tl is not None:
        nt = int(nt)
        _check_tensor('tiles', tl, ('N',), torch.int32, device)
        if not 0 <= nt <= tl.numel():
            raise _lib.PtmiError(f'tiles: the count must be in [0, {tl.numel()}], the length of the list')
    return tl, nt
