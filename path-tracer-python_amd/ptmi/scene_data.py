"""Compiled-scene container in the reference's array layout, and the packer
that turns it into the MI355X device layout of include/ptmi.h.

The reference compiles a scene into per-primitive-type numpy arrays
(src/render_server/taichi_renderer/scene_compiler.py:931-965) and a flattened
SAH BVH (bvh_compiler.py:132-168, sah_bvh_builder.py:338-418) and then
uploads them field by field (renderer.py:102-228). ``SceneArrays`` keeps
exactly those arrays (same names, dtypes and shapes) so fixtures captured from
the reference compare array-for-array; ``pack_device`` produces the packed
GPU layout (child-box BVH2 nodes, 16-float quads, 20-float materials, RGBA8
texels) documented in include/ptmi.h.
"""
from __future__ import annotations

import collections
import json
import os
from dataclasses import dataclass, field

import numpy as np

PRIM_SPHERE, PRIM_TRIANGLE, PRIM_QUAD = 0, 1, 2  # scene_compiler.py:10-12
MAX_IMAGES = 16


# What the host layer knows of one primitive kind: its name in the API (update_primitives' keyword, the renderer's
# ``primitives`` key) and its type code (bvh_prim_type, leaf codes, ids); the f32 per device row (include/ptmi.h) and
# per builder-form record ({c, r}; {v0, v1, v2}; {Q, u, v}) and the row columns such a record begins with; the
# attributes it goes by: geometry, materials and count on SceneArrays (the count also on DeviceLayout and the scene
# view), rows on DeviceLayout (and the view), tensor on DeviceScene; the class name the compiler and the renderer check.
PrimKind = collections.namedtuple('PrimKind', 'name code row_floats build_floats build_columns geometry materials '
                                              'count rows tensor class_name')
# one value per kind, in the only two orders there are:
ByCode = collections.namedtuple('ByCode', 'spheres triangles quads')  # prim_perm, row maps, leaf_of / dev_of, counts
ByStorage = collections.namedtuple('ByStorage', 'spheres quads tris')  # primitive_rows(), permute_rows(), prev_rows

# by type code; the columns are QUAD_COLUMNS' quad_Q .. quad_v and TRI_COLUMNS' triangle_v0 (below)
KINDS = (PrimKind('spheres', PRIM_SPHERE, 4, 4, slice(0, 4), 'sphere_data', 'sphere_mats', 'num_spheres', 'spheres',
                  't_spheres', 'Sphere'),
         PrimKind('triangles', PRIM_TRIANGLE, 12, 9, slice(0, 3), 'tris', 'tri_mats', 'num_triangles', 'tris',
                  't_tris', 'triangle'),
         PrimKind('quads', PRIM_QUAD, 16, 9, slice(4, 13), 'quads', 'quad_mats', 'num_quads', 'quads', 't_quads',
                  'quad'))
# the order of the device tensors, of the blocks of ``mats`` and of update_primitives' arguments
STORAGE = (KINDS[PRIM_SPHERE], KINDS[PRIM_QUAD], KINDS[PRIM_TRIANGLE])


def counts_by_code(obj):
    """ByCode of the primitive counts of a SceneArrays, a DeviceLayout or a scene view."""
    return ByCode(*(int(getattr(obj, k.count)) for k in KINDS))


def mat_bases(counts):
    """ByCode of the first ``mats`` row of each kind, for ByCode ``counts``: the blocks lie in storage order."""
    ends = np.cumsum([counts[k.code] for k in STORAGE])
    return ByCode(**{k.name: int(end) - counts[k.code] for k, end in zip(STORAGE, ends)})


# per-type material array names (compile_materials, scene_compiler.py:425-439)
MAT_KEYS = ('material_type', 'material_albedo', 'material_fuzz', 'material_ir', 'material_emit_color',
            'texture_type', 'texture_scale', 'texture_color1', 'texture_color2', 'texture_image_idx',
            'is_constant_medium', 'medium_density', 'medium_albedo')
BVH_KEYS = ('bvh_bbox_min', 'bvh_bbox_max', 'bvh_left_child', 'bvh_right_child', 'bvh_parent',
            'bvh_prim_type', 'bvh_prim_idx')
QUAD_KEYS = ('quad_Q', 'quad_u', 'quad_v', 'quad_normal', 'quad_D', 'quad_w')
TRI_KEYS = ('triangle_v0', 'triangle_v1', 'triangle_v2', 'triangle_edge1', 'triangle_edge2', 'triangle_normal')
PERLIN_KEYS = ('perlin_randvec', 'perlin_perm_x', 'perlin_perm_y', 'perlin_perm_z')

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'tests', 'golden')


def _empty_mats(n):
    return {
        'material_type': np.zeros(n, np.int32), 'material_albedo': np.zeros((n, 3), np.float32),
        'material_fuzz': np.zeros(n, np.float32), 'material_ir': np.zeros(n, np.float32),
        'material_emit_color': np.zeros((n, 3), np.float32), 'texture_type': np.zeros(n, np.int32),
        'texture_scale': np.ones(n, np.float32), 'texture_color1': np.zeros((n, 3), np.float32),
        'texture_color2': np.zeros((n, 3), np.float32), 'texture_image_idx': np.full(n, -1, np.int32),
        'is_constant_medium': np.zeros(n, np.int32), 'medium_density': np.zeros(n, np.float32),
        'medium_albedo': np.zeros((n, 3), np.float32),
    }


@dataclass
class SceneArrays:
    """Reference-layout compiled scene (geometry, materials, BVH, Perlin, images)."""
    sphere_data: np.ndarray
    sphere_mats: dict
    quads: dict
    quad_mats: dict
    tris: dict
    tri_mats: dict
    bvh: dict
    perlin: dict
    images: list = field(default_factory=list)  # (H, W, 3) uint8 each

    @property
    def num_spheres(self):
        return int(self.sphere_data.shape[0])

    @property
    def num_quads(self):
        return int(self.quads['quad_Q'].shape[0])

    @property
    def num_triangles(self):
        return int(self.tris['triangle_v0'].shape[0])

    @property
    def num_bvh_nodes(self):
        return int(self.bvh['bvh_bbox_min'].shape[0])

    def mats(self, prim_type):
        return getattr(self, KINDS[prim_type].materials)

    # ------------------------------------------------------------ constructors
    @classmethod
    def from_compiled(cls, geometry, materials, quad_geometry, quad_materials, tri_geometry, tri_materials,
                      bvh, perlin, images):
        """From compile_scene()/compile_bvh() outputs (reference or ptmi)."""
        ns = int(geometry['num_spheres'])
        nq = int(quad_geometry['num_quads'])
        nt = int(tri_geometry['num_triangles'])
        sd = np.asarray(geometry['sphere_data'], np.float32).reshape(ns, 4)
        q = {k: np.asarray(quad_geometry[k], np.float32).reshape((nq,) if k == 'quad_D' else (nq, 3))
             for k in QUAD_KEYS}
        t = {k: np.asarray(tri_geometry[k], np.float32).reshape(nt, 3) for k in TRI_KEYS}

        def fix(m, n):
            out = _empty_mats(n)
            for k in MAT_KEYS:
                if k in m:
                    out[k] = np.asarray(m[k], out[k].dtype).reshape(out[k].shape)
            return out

        b = {k: np.asarray(bvh[k], np.float32 if 'bbox' in k else np.int32) for k in BVH_KEYS}
        b['bvh_bbox_min'] = b['bvh_bbox_min'].reshape(-1, 3)
        b['bvh_bbox_max'] = b['bvh_bbox_max'].reshape(-1, 3)
        p = {'perlin_randvec': np.asarray(perlin['perlin_randvec'], np.float32).reshape(256, 3)}
        for k in PERLIN_KEYS[1:]:
            p[k] = np.asarray(perlin[k], np.int32).reshape(256)
        return cls(sd, fix(materials, ns), q, fix(quad_materials, nq), t, fix(tri_materials, nt), b, p,
                   [np.ascontiguousarray(im, dtype=np.uint8) for im in images])

    @classmethod
    def from_npz(cls, path, images=None):
        """Load a tests/golden/<scene>.npz fixture (see gen_fixtures.py)."""
        z = np.load(path)
        geom = {'sphere_data': z['sph_sphere_data'], 'num_spheres': z['sph_sphere_data'].shape[0]}
        mats = {k: z['sphm_' + k] for k in MAT_KEYS}
        qg = {k: z[k] for k in QUAD_KEYS}
        qg['num_quads'] = z['quad_Q'].shape[0]
        qm = {k: z['quadm_' + k] for k in MAT_KEYS}
        tg = {k: z[k] for k in TRI_KEYS}
        tg['num_triangles'] = z['triangle_v0'].shape[0]
        tm = {k: z['trim_' + k] for k in MAT_KEYS}
        bvh = {k: z[k] for k in BVH_KEYS}
        per = {k: z[k] for k in PERLIN_KEYS}
        if images is None:
            used = max(int(np.max(z['sphm_texture_image_idx'], initial=-1)),
                       int(np.max(z['quadm_texture_image_idx'], initial=-1)),
                       int(np.max(z['trim_texture_image_idx'], initial=-1)))
            images = [load_earthmap()] if used >= 0 else []
        return cls.from_compiled(geom, mats, qg, qm, tg, tm, bvh, per, images)


def golden_dir():
    return os.path.normpath(_GOLDEN)


def load_earthmap():
    """Decoded RGB8 earthmap (the only image texture the BASELINE scenes use)."""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'assets', 'earthmap_u8.npz'))['earthmap']


def load_fixture(name):
    return SceneArrays.from_npz(os.path.join(golden_dir(), name + '.npz'))


def fixture_camera(name, width):
    """f32 camera upload values captured from the reference (renderer.py:230-247)."""
    z = np.load(os.path.join(golden_dir(), name + '.npz'))
    tag = f'cam{width}_'
    cam = {k: np.asarray(z[tag + k], np.float32) for k in
           ('center', 'pixel00', 'delta_u', 'delta_v', 'defocus_u', 'defocus_v')}
    cam['defocus_angle'] = float(z[tag + 'defocus_angle'])
    cam['width'], cam['height'] = (int(v) for v in z[tag + 'size'])
    return cam


def camera_upload(cam):
    """f32 camera upload values (renderer.py:230-247) of an initialized camera
    object (ptmi.core.camera or the reference's), in fixture_camera's format."""
    def vec(p):
        return np.array([p.x, p.y, p.z], np.float64).astype(np.float32)
    return {'center': vec(cam.center), 'pixel00': vec(cam.pixel00_loc), 'delta_u': vec(cam.delta_u),
            'delta_v': vec(cam.delta_v), 'defocus_u': vec(cam.defocus_disk_u),
            'defocus_v': vec(cam.defocus_disk_v), 'defocus_angle': float(cam.defocus_angle),
            'width': int(cam.img_width), 'height': int(cam.img_height)}


def fixture_manifest():
    with open(os.path.join(golden_dir(), 'manifest.json')) as f:
        return json.load(f)


# ---------------------------------------------------------------- packing
LEAF_FLAG = np.int64(0x80000000)
LEAF_INDEX_BITS = 25  # leaf code: flag | type << 28 | material class << 25 | primitive index
MAX_PRIMS_PER_TYPE = 1 << LEAF_INDEX_BITS

# Material class of a leaf (include/ptmi.h PTMI_CLASS_*): which of the
# wavefront's shading lists a hit on it goes to, decided once per primitive
# from its material flags instead of by a dependent load after every traversal.
CLASS_LAMBERTIAN, CLASS_GLOSSY, CLASS_DIELECTRIC, CLASS_MEDIUM, CLASS_NOISE, CLASS_EMISSIVE = range(6)


NODE_FLOATS = 20  # 80-B internal node (include/ptmi.h)
NODE_BYTES = 4 * NODE_FLOATS  # an internal child ref is the child's byte offset in the node array
# Internal nodes sit in the node array in the reference's preorder. (A/B,
# rounds 1, 4 and 5, not kept: a 64-B stride without the stored x / y centres,
# breadth-first and depth-first sibling-pair placements; profiles/HISTORY.md §9d.)


def leaf_code(prim_type, prim_idx, mat_class=0):
    code = LEAF_FLAG | (np.int64(prim_type) << 28) | (np.int64(mat_class) << LEAF_INDEX_BITS) | np.int64(prim_idx)
    return np.int32(np.int64(code) - (1 << 32))  # as signed int32 bits


def material_class(flags):
    """Class of packed material flags (mt | tex << 4 | medium << 8 | ...):
    medium boundary; Perlin-textured Lambertian or isotropic (noise); then by
    material type: Lambertian 0, dielectric 2, emissive 3, else glossy (metal
    1, isotropic 4, unknown: scatter() decides)."""
    flags = np.asarray(flags, np.uint32).astype(np.int64)
    mt, tt, med = flags & 0xf, (flags >> 4) & 0xf, (flags >> 8) & 1
    cls = np.full(flags.shape, CLASS_GLOSSY, np.int64)
    cls[mt == 0] = CLASS_LAMBERTIAN
    cls[mt == 2] = CLASS_DIELECTRIC
    cls[mt == 3] = CLASS_EMISSIVE
    cls[(tt == 3) & ((mt == 0) | (mt == 4))] = CLASS_NOISE
    cls[med == 1] = CLASS_MEDIUM
    return cls


@dataclass
class DeviceLayout:
    """Host-side arrays in the device layout of include/ptmi.h."""
    nodes: np.ndarray       # (n_inner, node_bytes / 4) f32
    root_ref: int
    root_min: np.ndarray
    root_max: np.ndarray
    max_leaf_depth: int
    spheres: np.ndarray     # (ns, 4) f32
    quads: np.ndarray       # (nq, 16) f32
    tris: np.ndarray        # (nt, 12) f32
    mats: np.ndarray        # (ns+nq+nt, 20) f32
    texels: np.ndarray      # (sum H*W,) u32 RGBA8
    img_offset: list
    img_w: list
    img_h: list
    perlin_vec: np.ndarray  # (256, 4) f32
    perlin_perm: np.ndarray  # (768,) i32
    num_spheres: int
    num_quads: int
    num_triangles: int
    # a ByCode: device primitive k of type t is the reference's primitive prim_perm[t][k] (identity unless leaf_order)
    prim_perm: tuple = ()
    # the reference's own nodes for the stackless traversal (include/ptmi.h
    # ref_nodes): (num_bvh_nodes, 12) f32
    ref_nodes: np.ndarray = None

    @property
    def num_bvh_nodes(self):
        return 0 if self.ref_nodes is None else int(self.ref_nodes.shape[0])

    # internal nodes (the node array may hold unused padding rows besides)
    n_internal: int = None
    # enclosing medium shell hint (include/ptmi.h `shell`, find_shell), 0 = none
    shell: int = 0

    @property
    def n_inner(self):
        return int(self.nodes.shape[0]) if self.n_internal is None else int(self.n_internal)

    def nbytes(self):
        return sum(int(a.nbytes) for a in (self.nodes, self.spheres, self.quads, self.tris, self.mats,
                                              self.texels, self.perlin_vec, self.perlin_perm)
                   if a is not None) + (0 if self.ref_nodes is None else int(self.ref_nodes.nbytes))


# f32 columns of a mats row (include/ptmi.h) per reference-layout array; f32 19 is the flags word
MAT_FLOATS = 20
MAT_COLUMNS = {'material_albedo': slice(0, 3), 'material_fuzz': 3, 'material_emit_color': slice(4, 7),
               'material_ir': 7, 'texture_color1': slice(8, 11), 'texture_scale': 11,
               'texture_color2': slice(12, 15), 'medium_density': 15, 'medium_albedo': slice(16, 19)}


def mat_flags(rows):
    """The flags words (uint32) of (n, 20) f32 mats rows."""
    return np.ascontiguousarray(np.asarray(rows, np.float32)[:, MAT_FLOATS - 1]).view(np.uint32)


def unpack_mats(rows):
    """_pack_mats' inverse: the reference-layout material arrays (MAT_KEYS) of (n, 20) mats rows."""
    flags = mat_flags(rows).astype(np.int64)
    out = {key: rows[:, cols] for key, cols in MAT_COLUMNS.items()}
    out.update(material_type=(flags & 0xf).astype(np.int32), texture_type=((flags >> 4) & 0xf).astype(np.int32),
               is_constant_medium=((flags >> 8) & 1).astype(np.int32),
               texture_image_idx=((flags >> 16) - 1).astype(np.int32))
    return out


def _pack_mats(m, n):
    out = np.zeros((n, MAT_FLOATS), np.float32)
    for key, cols in MAT_COLUMNS.items():
        out[:, cols] = m[key]
    mt = m['material_type'].astype(np.int64)
    tt = m['texture_type'].astype(np.int64)
    if n and (mt.min() < 0 or mt.max() > 15 or tt.min() < 0 or tt.max() > 15):
        raise ValueError('material/texture type codes must be in [0, 15]')
    med = (m['is_constant_medium'] > 0).astype(np.int64)
    img = m['texture_image_idx'].astype(np.int64) + 1
    if n and (img.min() < 0 or img.max() > 0xffff):
        raise ValueError('texture image index out of range')
    flags = (mt | (tt << 4) | (med << 8) | (img << 16)).astype(np.uint32)
    out[:, 19] = flags.view(np.float32)
    return out


def leaf_depths(bvh):
    """Depth of every node (root = 0) of a preorder flattened BVH.

    The depths size the kernels' traversal stack, which has no overflow check,
    so a BVH whose children do not follow their parent (not the preorder
    flatten() of sah_bvh_builder.py:338-418 writes) is refused here rather
    than reported with too small a depth."""
    left, right = bvh['bvh_left_child'], bvh['bvh_right_child']
    n = left.shape[0]
    idx = np.arange(n)
    for name, ch in (('left', left), ('right', right)):
        has = ch >= 0
        if np.any(ch[has] >= n) or np.any(ch[has] <= idx[has]):
            raise ValueError(f'BVH is not in preorder: a {name} child does not follow its parent')
    depth = np.zeros(n, np.int32)
    for i in range(n):  # preorder: parents precede children
        if left[i] >= 0:
            depth[left[i]] = depth[i] + 1
        if right[i] >= 0:
            depth[right[i]] = depth[i] + 1
    return depth


def leaf_order_perm(bvh, counts):
    """ByCode, for ByCode ``counts``, of the reference's primitive indices in the order the
    preorder flattened BVH reaches their leaves (index order is preorder,
    sah_bvh_builder.py:338-418). Laying the device primitives and materials
    out in this order puts primitives that share a subtree, and are therefore
    tested by the same rays one after the other, on the same cache lines; the
    reference's compile order (scene_compiler.py:931) follows scene
    construction, which for vol2's 1000 randomly placed spheres is spatially
    random."""
    ptype, pidx = bvh['bvh_prim_type'], bvh['bvh_prim_idx']
    leaves = np.nonzero(pidx >= 0)[0]
    perm = []
    for t, n in enumerate(counts):
        order = pidx[leaves[ptype[leaves] == t]].astype(np.int64)
        if order.shape[0] != n or (n and not np.array_equal(np.sort(order), np.arange(n))):
            raise ValueError(f'BVH leaves of type {t} are not a permutation of the {n} primitives')
        perm.append(order)
    return ByCode(*perm)


def ref_layout_nodes(bvh, codes):
    """The reference's flattened nodes (fields.py:52-63, in its preorder) for
    the stackless traversal (traverse_bvh_stackless, kernels.py:453-597):
    12 f32 per node {min.xyz, left | max.xyz, right | parent, leaf code, side,
    0} (i32 bits). ``codes``: the device leaf code of every leaf (0 for
    internal nodes). ``side`` precomputes the reference's climb test
    ``0 if parent_node.left_child == node_idx else 1`` (kernels.py:506-507)."""
    left, right, parent = bvh['bvh_left_child'], bvh['bvh_right_child'], bvh['bvh_parent']
    n = left.shape[0]
    out = np.zeros((n, 12), np.float32)
    if n == 0:
        return out
    if np.any(parent[1:] < 0) or np.any(parent >= n) or parent[0] >= 0:
        raise ValueError('BVH parent pointers: only the root (node 0) may lack a parent')
    side = np.zeros(n, np.int32)
    has = parent >= 0
    side[has] = (left[parent[has]] != np.nonzero(has)[0]).astype(np.int32)
    out[:, 0:3] = bvh['bvh_bbox_min']
    out[:, 3] = left.astype(np.int32).view(np.float32)
    out[:, 4:7] = bvh['bvh_bbox_max']
    out[:, 7] = right.astype(np.int32).view(np.float32)
    out[:, 8] = parent.astype(np.int32).view(np.float32)
    out[:, 9] = np.asarray(codes, np.int32).view(np.float32)
    out[:, 10] = side.view(np.float32)
    return out


def node_slots(left, right, is_leaf):
    """Slot (row of the node array) of every internal node, by reference node
    index (-1 for leaves), in the reference's preorder, and the number of rows."""
    slot = np.full(left.shape[0], -1, np.int64)
    idx = np.nonzero(~is_leaf)[0]
    slot[idx] = np.arange(idx.shape[0])
    return slot, int(idx.shape[0])


def find_shell(sa: SceneArrays, max_leaf_depth: int):
    """The scene's enclosing medium shell (include/ptmi.h, ``shell``), as the
    reference BVH node index of its leaf, or -1: a constant-medium sphere of
    finite radius R > 0 whose leaf is not the root, with the farthest corner of
    every other leaf's box within R / 2 of its centre (float64), in a BVH of
    leaf depth <= 62. Of several, the largest. The "final scene" global fog
    (vol2: constant_medium(Sphere((0, 0, 0), 5000), 0.0001), the rest within
    0.2835 R) is one; a ray that starts within R / 2 of the centre and reaches
    the shell, or leaves it outwards, can hit nothing else on the way."""
    b = sa.bvh
    ptype, pidx = b['bvh_prim_type'], b['bvh_prim_idx']
    n = ptype.shape[0]
    if n < 3 or max_leaf_depth > 62:
        return -1
    leaves = np.nonzero(pidx >= 0)[0]
    bmin = b['bvh_bbox_min'][leaves].astype(np.float64)
    bmax = b['bvh_bbox_max'][leaves].astype(np.float64)
    med = np.asarray(sa.sphere_mats['is_constant_medium']) > 0
    best, best_r = -1, 0.0
    for k, node in enumerate(leaves):
        if node == 0 or ptype[node] != PRIM_SPHERE or not med[pidx[node]]:
            continue
        c = sa.sphere_data[pidx[node], :3].astype(np.float64)
        r = float(sa.sphere_data[pidx[node], 3])
        if not (np.isfinite(r) and r > 0.0 and np.all(np.isfinite(c))):
            continue
        far = np.sqrt(np.sum(np.maximum(np.abs(bmin - c), np.abs(bmax - c)) ** 2, axis=1))
        far[k] = 0.0
        if np.all(far <= 0.5 * r) and r > best_r:
            best, best_r = int(node), r
    return best


# f32 columns of a device row (include/ptmi.h) per reference-layout array: the one table of both directions
QUAD_COLUMNS = {'quad_normal': slice(0, 3), 'quad_D': 3, 'quad_Q': slice(4, 7), 'quad_u': slice(7, 10),
                'quad_v': slice(10, 13), 'quad_w': slice(13, 16)}
TRI_COLUMNS = {'triangle_v0': slice(0, 3), 'triangle_edge1': slice(3, 6), 'triangle_edge2': slice(6, 9),
               'triangle_normal': slice(9, 12)}


def _pack_rows(arrays, columns, width):
    rows = np.zeros((arrays[next(iter(columns))].shape[0], width), np.float32)
    for key, cols in columns.items():
        rows[:, cols] = arrays[key]
    return rows


def pack_quads(q):
    """Device rows (include/ptmi.h: 16 f32) of reference-layout quad arrays (QUAD_KEYS), in their order."""
    return _pack_rows(q, QUAD_COLUMNS, KINDS[PRIM_QUAD].row_floats)


def pack_tris(t):
    """Device rows (12 f32) of reference-layout triangle arrays (TRI_KEYS), in their order."""
    return _pack_rows(t, TRI_COLUMNS, KINDS[PRIM_TRIANGLE].row_floats)


def unpack_quads(rows):
    """pack_quads' inverse: the reference-layout arrays (QUAD_KEYS) of (n, 16) device rows."""
    return {key: rows[:, cols] for key, cols in QUAD_COLUMNS.items()}


def unpack_tris(rows, build):
    """pack_tris' inverse: the reference-layout arrays (TRI_KEYS) of (n, 12) device
    rows and their (n, 9) builder-form records {v0, v1, v2}; a row holds edges, not v1 and v2."""
    return dict({key: rows[:, cols] for key, cols in TRI_COLUMNS.items()},
                triangle_v1=build[:, 3:6], triangle_v2=build[:, 6:9])


def fill_node_boxes(nodes, rows, bmin, bmax, l, r):
    """The box part of node rows ``rows`` (include/ptmi.h): the boxes of the
    children ``l`` and ``r`` interleaved per component, and their centres. The
    two refs (f32 12, 13) are not touched."""
    nodes[rows, 0:12:2] = np.concatenate([bmin[l], bmax[l]], axis=1)
    nodes[rows, 1:12:2] = np.concatenate([bmin[r], bmax[r]], axis=1)
    # box centres (min + max) * 0.5 in f32 — the same rounding as the
    # kernels' (kernels.py:707-710), so precomputing them changes nothing
    cl = (bmin[l] + bmax[l]) * np.float32(0.5)
    cr = (bmin[r] + bmax[r]) * np.float32(0.5)
    nodes[rows, 14], nodes[rows, 15] = cl[:, 2], cr[:, 2]
    nodes[rows, 16], nodes[rows, 17] = cl[:, 0], cr[:, 0]
    nodes[rows, 18], nodes[rows, 19] = cl[:, 1], cr[:, 1]


def shell_hint(sa: SceneArrays, slot, max_leaf_depth: int, node_bytes: int = NODE_BYTES) -> int:
    """The ``shell`` value of include/ptmi.h for find_shell's leaf: 1 + the byte
    offset of the node holding the shell's leaf as a child + the child index;
    0 without a shell. ``slot``: node_slots' rows."""
    leaf = find_shell(sa, max_leaf_depth)
    if leaf <= 0:
        return 0
    par = int(sa.bvh['bvh_parent'][leaf])
    return 1 + int(slot[par]) * node_bytes + (0 if int(sa.bvh['bvh_left_child'][par]) == leaf else 1)


def pack_device(sa: SceneArrays, node_bytes: int = NODE_BYTES, leaf_order: bool = True) -> DeviceLayout:
    """Reference-layout arrays -> include/ptmi.h device layout. ``node_bytes``
    is the library's node stride (ptmi_node_bytes(): 80, one child record
    per internal node). Each leaf code carries its primitive's material
    class (material_class). ``leaf_order`` renumbers each primitive type in BVH leaf order
    (leaf_order_perm); leaf codes, primitive and material rows are permuted
    together, so every lookup the kernels make finds the same data and the
    traversal visits the same leaves in the same order: results are
    unchanged bit for bit."""
    ns, nq, nt = sa.num_spheres, sa.num_quads, sa.num_triangles
    b = sa.bvh
    bmin, bmax = b['bvh_bbox_min'], b['bvh_bbox_max']
    left, right = b['bvh_left_child'], b['bvh_right_child']
    ptype, pidx = b['bvh_prim_type'], b['bvh_prim_idx']
    n = bmin.shape[0]
    if n != (2 * (ns + nq + nt) - 1 if (ns + nq + nt) else 0):
        raise ValueError(f'BVH has {n} nodes for {ns + nq + nt} primitives (expected 2N-1)')
    is_leaf = pidx >= 0
    internal = np.nonzero(~is_leaf)[0]
    if np.any(left[internal] < 0) or np.any(right[internal] < 0):
        raise ValueError('internal BVH node with a missing child')
    counts = counts_by_code(sa)
    perm = leaf_order_perm(b, counts) if leaf_order and n else ByCode(*(np.arange(c, dtype=np.int64) for c in counts))
    new_idx = pidx.astype(np.int64).copy()
    for t in range(3):
        sel = is_leaf & (ptype == t)
        new_idx[sel] = np.argsort(perm[t])[pidx[sel]]  # the permutation's inverse
    if max(counts) > MAX_PRIMS_PER_TYPE:
        raise ValueError(f'at most {MAX_PRIMS_PER_TYPE} primitives of one type (25-bit leaf index)')
    mats = np.concatenate([_pack_mats(sa.mats(k.code), counts[k.code])[perm[k.code]] for k in STORAGE], axis=0)
    mat_base = np.array(mat_bases(counts), np.int64)
    cls = np.zeros(n, np.int64)
    if n:
        rows = mat_base[np.where(is_leaf, ptype, 0)] + np.where(is_leaf, new_idx, 0)
        cls = np.where(is_leaf, material_class(mats[rows, 19].view(np.uint32)) if len(mats) else 0, 0)
    codes = ((LEAF_FLAG | (ptype.astype(np.int64) << 28) | (cls << LEAF_INDEX_BITS) | new_idx)
             - (1 << 32)).astype(np.int32)
    if node_bytes != NODE_BYTES:
        raise ValueError(f'unsupported node stride {node_bytes} (the library reads {NODE_BYTES}-B nodes)')
    cidx, nrows = node_slots(left, right, is_leaf)
    if nrows * node_bytes > 0x7fffffff:
        raise ValueError(f'{nrows} BVH node rows: byte offsets exceed int32')
    refs = np.where(is_leaf, codes, (cidx * node_bytes).astype(np.int32)).astype(np.int32)
    nodes = np.zeros((nrows, node_bytes // 4), np.float32)
    if internal.size:
        l, r = left[internal], right[internal]
        rows = cidx[internal]
        fill_node_boxes(nodes, rows, bmin, bmax, l, r)
        nodes[rows, 12] = refs[l].view(np.float32)
        nodes[rows, 13] = refs[r].view(np.float32)
    ref_nodes = ref_layout_nodes(b, np.where(is_leaf, codes, 0).astype(np.int32))
    if n:
        root_ref = int(refs[0])
        root_min, root_max = bmin[0].copy(), bmax[0].copy()
        max_leaf_depth = int(leaf_depths(b).max())
    else:
        root_ref, root_min, root_max, max_leaf_depth = 0, np.zeros(3, np.float32), np.zeros(3, np.float32), 0
    shell = shell_hint(sa, cidx, max_leaf_depth, node_bytes)
    spheres = np.ascontiguousarray(np.asarray(sa.sphere_data, np.float32).reshape(ns, 4)[perm.spheres])
    quads, tris = pack_quads(sa.quads)[perm.quads], pack_tris(sa.tris)[perm.triangles]
    if len(sa.images) > MAX_IMAGES:
        raise ValueError(f'at most {MAX_IMAGES} image textures')
    texels, offs, ws, hs, off = [], [], [], [], 0
    for im in sa.images:
        h, w, _ = im.shape
        rgba = np.zeros((h, w, 4), np.uint8)
        rgba[..., :3] = im
        texels.append(rgba.reshape(-1).view(np.uint32))
        offs.append(off)
        ws.append(w)
        hs.append(h)
        off += h * w
    texels = np.concatenate(texels) if texels else np.zeros(1, np.uint32)
    pv = np.zeros((256, 4), np.float32)
    pv[:, :3] = sa.perlin['perlin_randvec']
    pperm = np.concatenate([sa.perlin['perlin_perm_x'], sa.perlin['perlin_perm_y'],
                            sa.perlin['perlin_perm_z']]).astype(np.int32)
    if pperm.min() < 0 or pperm.max() > 255:
        raise ValueError('Perlin permutation out of range')
    return DeviceLayout(nodes, root_ref, root_min, root_max, max_leaf_depth, spheres, quads, tris, mats,
                        texels, offs, ws, hs, pv, pperm, ns, nq, nt, perm, ref_nodes, int(internal.shape[0]), shell)


def compile_world(world, perlin_tables=None):
    """World -> SceneArrays the way the renderer does it (renderer.py:65-100):
    Perlin tables from a perlin() created after the scene (it draws from the
    global `random` stream), compile_scene, native SAH BVH, RGB8 images."""
    from . import bvh as bvh_mod, core, scene_compiler
    if perlin_tables is None:
        perlin_tables = core.perlin().tables()
    (geom, mats, spheres, qgeom, qmats, quads, tgeom, tmats, tris, _reg,
     img_list) = scene_compiler.compile_scene(world)
    bvh = bvh_mod.compile_bvh(world, spheres, quads, tris)
    return SceneArrays.from_compiled(geom, mats, qgeom, qmats, tgeom, tmats, bvh, perlin_tables,
                                     [scene_compiler.image_u8(t) for t in img_list])
