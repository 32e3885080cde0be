"""GPU test of what the three scene-edit calls share on the device (csrc/pt_edit_lists.hpp,
DESIGN.md §19): the selection of a lane's list and entry when one of the three lists is empty in
each position, and when a 256-lane block ends inside the last list behind an empty one. Every call
is checked against its own reference, byte for byte, and must change exactly as many rows as it
was given edits."""
import numpy as np
import pytest

import material_helpers as mh
import parity_helpers as ph
import pose_helpers as psh
import update_helpers as uh
from ptmi import pose, scene_data as sd

pytestmark = pytest.mark.gpu
f32 = np.float32
WIDTH = 48
T = 1.0 / 3.0
KINDS = ('spheres', 'quads', 'triangles')
ROWS = {'spheres': 'spheres', 'quads': 'quads', 'triangles': 'tris'}  # the kind's member of a device image
TENSORS = ('nodes', 'ref_nodes', 'spheres', 'quads', 'tris')
# (spheres, quads, triangles): a list empty in each position, one entry in the last list alone, and
# 257 entries whose 256th lane lies in the last list behind an empty one
PATTERNS = [(2, 0, 3), (0, 2, 3), (2, 3, 0), (0, 0, 1), (3, 0, 254)]

_cases = {}


def case(pattern):
    """The coverage scene, its untouched device image, and for a pattern the tracks of its first primitives of
    every kind and their records posed at T (update_primitives' arguments). Made once."""
    if 'sa' not in _cases:
        sa = ph.fixture('coverage', WIDTH)
        assert sa.num_spheres >= 3 and sa.num_quads >= 3 and sa.num_triangles >= 254
        _cases['sa'] = sa
        _cases['rest'] = psh.device_image(new_scene(sa))
    if pattern not in _cases:
        s, q, t = pattern
        tracks = psh.scene_tracks('coverage', WIDTH, spheres=range(s), quads=range(q), triangles=range(t),
                                  seed=sum(pattern), reach=0.5)
        assert tuple(len(tracks[k]) for k in KINDS) == pattern
        _cases[pattern] = (tracks, pose.posed_records(tracks, T))
    return (_cases['sa'], _cases['rest']) + _cases[pattern]


def new_scene(sa):
    from ptmi import device
    return device.DeviceScene.from_arrays(sa)


def changed_rows(got, rest, keys):
    """How many rows of each member differ in any bit."""
    return tuple(int((got[k].view(np.uint32) != rest[k].view(np.uint32)).any(axis=1).sum()) for k in keys)


@pytest.mark.parametrize('pattern', PATTERNS)
def test_update_with_an_empty_list_in_each_position(pattern):
    sa, rest, _, records = case(pattern)
    ds = new_scene(sa)
    ds.update_primitives(*records)
    got = psh.device_image(ds)
    want = sd.pack_device(uh.refit(sa, psh.as_edits(records)))
    for k in TENSORS:
        assert got[k].tobytes() == np.asarray(getattr(want, k), f32).tobytes(), k
    assert changed_rows(got, rest, ROWS.values()) == pattern
    assert psh.images_differ(got, rest, ('mats', 'texels')) == []


@pytest.mark.parametrize('pattern', PATTERNS)
def test_pose_with_an_empty_list_in_each_position(pattern):
    sa, rest, tracks, records = case(pattern)
    ds, other = new_scene(sa), new_scene(sa)
    ds.set_tracks(*pose.track_records(tracks))
    ds.pose(T)
    other.update_primitives(*records)
    got = psh.device_image(ds)
    assert psh.images_differ(got, psh.device_image(other), TENSORS + ('view_root',)) == []
    assert changed_rows(got, rest, ROWS.values()) == pattern
    assert psh.images_differ(got, rest, ('mats', 'texels')) == []


@pytest.mark.parametrize('pattern', PATTERNS)
def test_materials_with_an_empty_list_in_each_position(pattern):
    sa, rest = case(pattern)[:2]
    walk = [row for _, row in mh.class_walk(len(sa.images))]
    edits = {}
    for kind, n in zip(KINDS, pattern):
        if n:  # every primitive gets a row of the class walk that is not the one it has
            now = mh.rows_of(sa, kind)[:n]
            rows = [next(r for r in walk[i % len(walk):] + walk if r.tobytes() != now[i].tobytes()) for i in range(n)]
            edits[kind] = (np.arange(n), np.stack(rows))
    ds = new_scene(sa)
    ds.update_materials(**edits)
    got = psh.device_image(ds)
    want = sd.pack_device(mh.apply(sa, edits))
    for k in TENSORS + ('mats',):
        assert got[k].tobytes() == np.asarray(getattr(want, k), f32).tobytes(), k
    assert changed_rows(got, rest, ('mats',)) == (sum(pattern),)
    assert psh.images_differ(got, rest, ('spheres', 'quads', 'tris', 'texels')) == []
