"""ctypes binding of the material-edit ABI (include/ptmi_material.h): material
rows of a resident scene replaced in place on the device, and the material
class in the leaf codes patched with them.

The entry point lives in the same libptmi.so as the integrator's and is loaded
through ``_lib.load()``; its signature table is kept here and bound by
``_lib.bind``.

``DeviceScene.update_materials`` (ptmi.device) is the caller, and its numpy
halves are here: ``check_edits`` and ``refresh_mirror``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .scene_data import (KINDS, LEAF_INDEX_BITS, MAT_FLOATS, NODE_BYTES, STORAGE, mat_bases, mat_flags,
                         material_class, shell_hint, unpack_mats)
from .update import check_indices

MATERIAL_VERSION = 1  # PTMI_MATERIAL_VERSION of include/ptmi_material.h
CLASS_MASK = 7 << LEAF_INDEX_BITS  # the material class of a leaf code, bits 25 - 27


class MaterialList(C.Structure):
    """ptmi_material_list."""
    _fields_ = [('prim', C.c_void_p), ('leaf', C.c_void_p), ('row', C.c_void_p), ('count', C.c_int32)]


def _signatures():
    """Every export of include/ptmi_material.h: name -> (restype, argtypes)."""
    P = C.c_void_p
    L = C.POINTER(MaterialList)
    return {
        'ptmi_update_materials': (C.c_int, [C.POINTER(_lib.SceneView), L, L, L, P, P]),
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def load():
    """libptmi.so (``_lib.load()``) with the material export bound; a library
    without it raises PtmiError."""
    return _lib.bind(_lib.load(), SIGNATURES)


def check_edits(counts, num_images, spheres=None, quads=None, triangles=None):
    """update_materials' arguments checked against the ByCode ``counts`` and the scene's number of images:
    {type code: (int64 indices, (n, 20) f32 rows)} of the non-empty ones. A ValueError otherwise."""
    edits = {}
    for k, arg in zip(STORAGE, (spheres, quads, triangles)):
        if arg is None:
            continue
        name, count = k.name, counts[k.code]
        idx, rows = arg
        idx = check_indices(name, idx, count)
        n = int(idx.size)
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.size != n * MAT_FLOATS:
            raise ValueError(f'{name}: rows must be (n, {MAT_FLOATS}) f32')
        rows = rows.reshape(n, MAT_FLOATS)
        if not np.isfinite(rows[:, :MAT_FLOATS - 1]).all():
            raise ValueError(f'{name}: the 19 values before the flags word must be finite')
        flags = mat_flags(rows).astype(np.int64)
        if n and np.any(flags & 0xfe00):
            raise ValueError(f'{name}: bits 9 - 15 of a flags word must be zero')
        if n and int((flags >> 16).max()) > int(num_images):
            raise ValueError(f'{name}: a flags word names image {int((flags >> 16).max()) - 1}, the scene has '
                             f'{int(num_images)}')
        if n:
            edits[k.code] = (idx, rows)
    return edits


def patch_codes(codes, classes):
    """int32 leaf codes with their class bits (25 - 27) replaced by ``classes``; nothing else changes."""
    words = np.asarray(codes, np.int32).view(np.uint32).astype(np.int64)
    out = (words & ~np.int64(CLASS_MASK)) | (np.asarray(classes, np.int64) << LEAF_INDEX_BITS)
    return out.astype(np.uint32).view(np.int32)


def refresh_mirror(sa, lay, maps, edits, node_bytes=NODE_BYTES):
    """A scene's SceneArrays and DeviceLayout, in place, after a finished material edit: the material arrays
    and ``mats`` rows from ``check_edits``' edits, the class bits of the edited primitives' leaf codes in
    ``ref_nodes``, in the parents' ``nodes`` rows and, where the root is a leaf, in ``root_ref``, and the shell
    hint evaluated anew. ``maps``: ``update.index_maps`` of the tree."""
    bases = mat_bases([getattr(lay, k.count) for k in KINDS])
    parent, left = sa.bvh['bvh_parent'], sa.bvh['bvh_left_child']
    ref_words, node_words = lay.ref_nodes.view(np.int32), lay.nodes.view(np.int32)
    for t, (idx, rows) in edits.items():
        mirror = getattr(sa, KINDS[t].materials)
        for key, values in unpack_mats(rows).items():
            mirror[key][idx] = values
        lay.mats[bases[t] + maps['dev_of'][t][idx]] = rows
        leaves = maps['leaf_of'][t][idx]
        codes = patch_codes(ref_words[leaves, 9], material_class(mat_flags(rows)))
        ref_words[leaves, 9] = codes
        par = parent[leaves]
        has = par >= 0
        side = (left[par[has]] != leaves[has]).astype(np.int64)
        node_words[maps['slot_np'][par[has]], 12 + side] = codes[has]
        if not has.all():  # the root is a leaf: a one-primitive scene
            lay.root_ref = int(codes[~has][0])
    lay.shell = shell_hint(sa, maps['slot_np'], lay.max_leaf_depth, node_bytes)
