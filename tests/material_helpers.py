"""numpy reference of the material-edit ABI (include/ptmi_material.h).

``apply(sa, edits)`` gives a new SceneArrays whose material arrays carry the
edits; ``pack_device`` of the result, on the same BVH, is the expected device
image (the packer computes every leaf code's class from the flags anew), and
the oracle renders from it.

``edits`` maps 'spheres' / 'quads' / 'triangles' to ``(reference primitive
indices, (n, 20) f32 mats rows)``, the arguments of
``DeviceScene.update_materials``. The row layout is written out here once
more, apart from the package's table, so that the two check each other."""
import dataclasses

import numpy as np

f32 = np.float32
MATS = {'spheres': 'sphere_mats', 'quads': 'quad_mats', 'triangles': 'tri_mats'}
LAMBERTIAN, METAL, DIELECTRIC, EMISSIVE, ISOTROPIC = range(5)
SOLID, CHECKER, IMAGE, NOISE = range(4)
CLASS = {'lambertian': 0, 'glossy': 1, 'dielectric': 2, 'medium': 3, 'noise': 4, 'emissive': 5}


def flags_word(mat_type, tex_type=SOLID, medium=0, image=-1):
    return np.uint32(mat_type | tex_type << 4 | (1 if medium else 0) << 8 | (image + 1) << 16)


def row(mat_type, tex_type=SOLID, albedo=(0, 0, 0), fuzz=0.0, emit=(0, 0, 0), ir=1.0, color1=(0, 0, 0), scale=1.0,
        color2=(0, 0, 0), medium=0, density=0.0, medium_albedo=(0, 0, 0), image=-1):
    """One mats row (include/ptmi.h): {albedo.xyz, fuzz | emit.xyz, ir | color1.xyz, tex_scale | color2.xyz,
    density | medium_albedo.xyz, flags}."""
    r = np.zeros(20, f32)
    r[0:3], r[3], r[4:7], r[7] = albedo, fuzz, emit, ir
    r[8:11], r[11], r[12:15], r[15], r[16:19] = color1, scale, color2, density, medium_albedo
    r[19:20] = np.array([flags_word(mat_type, tex_type, medium, image)], np.uint32).view(f32)
    return r


def flags_of(rows):
    return np.ascontiguousarray(np.asarray(rows, f32).reshape(-1, 20)[:, 19]).view(np.uint32)


def rows_of(sa, name):
    """The mats rows, in reference order, of every primitive of a kind."""
    m = getattr(sa, MATS[name])
    n = len(m['material_type'])
    out = np.zeros((n, 20), f32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = (m['material_albedo'], m['material_fuzz'],
                                                      m['material_emit_color'], m['material_ir'])
    out[:, 8:11], out[:, 11], out[:, 12:15] = m['texture_color1'], m['texture_scale'], m['texture_color2']
    out[:, 15], out[:, 16:19] = m['medium_density'], m['medium_albedo']
    fl = (m['material_type'].astype(np.int64) | m['texture_type'].astype(np.int64) << 4
          | (m['is_constant_medium'] > 0).astype(np.int64) << 8 | (m['texture_image_idx'].astype(np.int64) + 1) << 16)
    out[:, 19] = fl.astype(np.uint32).view(f32)
    return out


def current(sa, name, idx):
    """The edit that writes back what ``sa`` holds for primitives ``idx``: the inverse of any edit of them."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    return idx, rows_of(sa, name)[idx]


def apply(sa, edits):
    """A new SceneArrays: ``sa`` with the material arrays edited. Geometry, BVH, Perlin tables and images are
    shared with ``sa`` and not written."""
    new = {attr: {k: np.array(v) for k, v in getattr(sa, attr).items()} for attr in MATS.values()}
    for name, (idx, rows) in edits.items():
        m = new[MATS[name]]
        idx = np.asarray(idx, np.int64).reshape(-1)
        rows = np.asarray(rows, f32).reshape(len(idx), 20)
        fl = flags_of(rows).astype(np.int64)
        m['material_albedo'][idx], m['material_fuzz'][idx] = rows[:, 0:3], rows[:, 3]
        m['material_emit_color'][idx], m['material_ir'][idx] = rows[:, 4:7], rows[:, 7]
        m['texture_color1'][idx], m['texture_scale'][idx] = rows[:, 8:11], rows[:, 11]
        m['texture_color2'][idx], m['medium_density'][idx] = rows[:, 12:15], rows[:, 15]
        m['medium_albedo'][idx] = rows[:, 16:19]
        m['material_type'][idx], m['texture_type'][idx] = fl & 0xf, (fl >> 4) & 0xf
        m['is_constant_medium'][idx], m['texture_image_idx'][idx] = (fl >> 8) & 1, (fl >> 16) - 1
    return dataclasses.replace(sa, **new)


def mats_equal(a, b):
    """Byte and dtype equality of the three material dicts of two SceneArrays."""
    return all(np.asarray(getattr(a, attr)[k]).tobytes() == np.asarray(getattr(b, attr)[k]).tobytes()
               and np.asarray(getattr(a, attr)[k]).dtype == np.asarray(getattr(b, attr)[k]).dtype
               for attr in MATS.values() for k in getattr(a, attr))


def class_walk(num_images=0):
    """(class name, row) pairs that walk every material class and every way into it: Lambertian solid /
    checker / resident image (if the scene has one), Lambertian noise and isotropic noise (NOISE), metal and
    isotropic solid (GLOSSY), dielectric, emissive, and a medium boundary over a dielectric and over a noise
    Lambertian (medium wins)."""
    walk = [
        ('lambertian', row(LAMBERTIAN, albedo=(.2, .6, .3), color1=(.2, .6, .3), color2=(.2, .6, .3))),
        ('lambertian', row(LAMBERTIAN, CHECKER, albedo=(1, 1, 1), color1=(.9, .9, .9), color2=(.2, .3, .1), scale=0.32)),
        ('noise', row(LAMBERTIAN, NOISE, albedo=(1, 1, 1), color1=(.5, .5, .5), color2=(.5, .5, .5), scale=4.0)),
        ('glossy', row(METAL, albedo=(.8, .6, .2), fuzz=0.25, color1=(.8, .6, .2), color2=(.8, .6, .2))),
        ('dielectric', row(DIELECTRIC, albedo=(1, 1, 1), ir=1.5, color1=(1, 1, 1), color2=(1, 1, 1))),
        ('emissive', row(EMISSIVE, emit=(3, 2.5, 2))),
        ('noise', row(ISOTROPIC, NOISE, albedo=(.7, .7, .7), color1=(.5, .5, .5), color2=(.5, .5, .5), scale=2.0)),
        ('glossy', row(ISOTROPIC, albedo=(.6, .6, .8), color1=(.6, .6, .8), color2=(.6, .6, .8))),
        ('medium', row(DIELECTRIC, albedo=(1, 1, 1), ir=1.5, color1=(1, 1, 1), color2=(1, 1, 1), medium=1,
                       density=0.4, medium_albedo=(.8, .8, .9))),
        ('medium', row(LAMBERTIAN, NOISE, albedo=(1, 1, 1), color1=(.5, .5, .5), color2=(.5, .5, .5), medium=1,
                       density=0.2, medium_albedo=(.3, .3, .3))),
    ]
    if num_images:
        walk.insert(2, ('lambertian', row(LAMBERTIAN, IMAGE, albedo=(1, 1, 1), color1=(1, 1, 1), color2=(1, 1, 1),
                                          image=num_images - 1)))
    return walk


def walk_edits(sa, offset=0, stride=1):
    """Edits that give primitive i of every kind the class walk's row (i + offset) mod its length, for every
    ``stride``-th primitive: a set that moves primitives of all three types through every class."""
    walk = class_walk(len(sa.images))
    out = {}
    for k, (name, attr) in enumerate(MATS.items()):
        n = len(getattr(sa, attr)['material_type'])
        idx = np.arange(0, n, stride, dtype=np.int64)
        if idx.size:
            out[name] = (idx, np.stack([walk[(int(i) + offset + 3 * k) % len(walk)][1] for i in idx]))
    return out


def classes_of(edits):
    """The set of material classes (PTMI_CLASS_*) the rows of ``edits`` have, by the package's function."""
    from ptmi import scene_data as sd
    return {int(c) for _, rows in edits.values() for c in sd.material_class(flags_of(rows))}
