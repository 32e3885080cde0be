"""MI355X renderer with the reference's TaichiRenderer surface.

Mirrors src/render_server/taichi_renderer/renderer.py:25-648 — constructor
``(world, cam, img_path)``, ``max_depth`` / ``background_color`` attributes
picked up at render time, ``render()`` (megakernel), ``render_wavefront()``,
the InteractiveViewer compatibility API (``render_sample``,
``clear_accumulation_buffer``, ``_upload_camera_to_gpu``, ``write_image``,
``print_statistics``, ``num_spheres``, ``num_bvh_nodes``, ``timing``,
``sample_times``, ``current_sample``) — on the HIP integrator of libptmi.

Differences by design: no Taichi JIT (``timing['taichi_init']`` stays 0),
scene arrays sized dynamically (no MAX_* capacities), each
renderer owns its device buffers (the reference's are module globals), the
random stream is keyed by (seed, pixel, sample) so ``render_sample(i)``
renders sample i deterministically, and the preview window is not opened
(Tk GUI is out of scope): ``enable_preview`` is accepted and ignored.

Checkpoint / resume (the reference has none: its progressive accumulation
lives only in accum_buffer, renderer.py:405-442):
``save_checkpoint(path)`` writes the accumulator, the next sample index and
the render state; ``load_checkpoint(path)`` followed by ``render(resume=True)``
finishes the remaining samples. Samples are keyed by (seed, pixel, sample) and
added in sample order, so the resumed image is bit-identical to an
uninterrupted render.

Adaptive sampling (no counterpart in the reference either): ``render_adaptive``
keeps per-pixel {n, mean, M2} of the sample luminance next to the accumulator
and renders passes of the 64-pixel tiles whose error estimate is still above
a target; ``noise_map()`` / ``sample_count_map()`` expose the estimates, the
image divides each pixel by its own sample count, and checkpoints carry the
extra state.

Denoising (no counterpart in the reference): after a ``render_adaptive``,
``denoise`` filters the accumulator by the per-pixel error estimates into
``denoised``; ``image_u8(denoised=True)`` / ``write_denoised_image`` give the
8-bit result. ``denoise(guided=True)`` adds first-hit normal,
depth and albedo guides as edge-stopping terms; ``guides()`` / ``guide_maps()``
give them as a tensor or as numpy AOVs. Derived data: not
checkpointed.

Temporal reprojection (no counterpart in the reference):
``reproject_history(prev_camera, prev_guides)`` carries the accumulator and
the stats of a stats render to the camera uploaded since, by the guides of both
cameras; InteractiveViewer(temporal=True) does so on every
camera move. Derived state: not checkpointed.

Scene updates (no counterpart in the reference): ``update_primitives`` moves
spheres, quads and triangles of the resident scene and refits the BVH on the
device instead of building a new renderer; ``primitives`` lists
the objects by the indices it takes. The image starts over. ``tree_growth()``
says how far the refit tree's boxes have grown since it was built, and
``rebuild_bvh()`` / ``update_primitives(rebuild=True | 'auto')`` rebuild the
BVH of the resident scene in place, history included.
``update_materials`` replaces materials of the resident scene: a dimmed light,
a recoloured wall, a diffuse ball turned to glass, a thicker fog (DESIGN.md
§22).

History validation (no counterpart in the reference): ``render_validated(spp)``
renders a few fresh samples apart from the carried history, drops the history
where a window of pixels says the light has changed (a moved shadow, a
reflection) and merges the rest;
InteractiveViewer(temporal=True, validate=True) does so after every
reprojecting restart. Derived state: not checkpointed.

Motion blur (the reference's Taichi kernels render ``Sphere.moving`` frozen at
t = 0, quirk Q22; its CPU renderers blur): with ``shutter=(t0, t1)`` every
render call traces each slice of ``slice_spp`` samples with the moving
primitives posed at that slice's shutter time (ptmi.pose) and
leaves the device at the rest scene. Moving spheres are tracked by themselves;
``set_motion`` gives quads and triangles a displacement, and ``set_bodies``
makes groups of primitives rigid bodies that turn about an axis and move
(ptmi.rigid). ``shutter=None``, the default, renders as before
and makes no pose call.
"""
from __future__ import annotations

import copy
import dataclasses
import os
import time

import numpy as np
import torch

from . import _lib, build as build_mod, bvh as bvh_mod, core, device, pose as pose_mod, rigid as rigid_mod, scene_compiler, tree as tree_mod
from .scene_data import STORAGE, SceneArrays

# kernels.py:746: the reference's switch between its front-to-back stack
# traversal (False, its default) and its parent-pointer stackless traversal.
# Read when a renderer uploads its camera; the per-renderer attribute
# `use_stackless_traversal` overrides it.
USE_STACKLESS_TRAVERSAL = False


@dataclasses.dataclass
class _History:
    """What a rendered history was seen with: the camera (a camera-upload dict
    or ptmi_camera) and the guides of its frame and, for a scene updated since,
    the id image of that frame (``guides_ids()``) and the primitive rows of its
    scene (``DeviceScene.primitive_rows()``). One render, one scene revision."""
    camera: object
    guides: object
    ids: object = None
    rows: object = None


class MI355XRenderer:
    def __init__(self, world, cam, img_path: str, seed: int = 0, samples_per_launch: int = 0, device_id=None,
                 shutter=None, slice_spp=pose_mod.SLICE_SPP):
        self.timing = {'taichi_init': 0.0, 'scene_compile': 0.0, 'bvh_compile': 0.0, 'bvh_flatten': 0.0,
                       'camera_upload': 0.0, 'gpu_upload': 0.0, 'kernel_warmup': 0.0, 'total_setup': 0.0}
        self.sample_times = []
        self.current_sample = 0
        self.render_start_time = 0.0
        t_setup = time.time()
        self.img_path = img_path
        self.cam = cam
        self.cam.initialize()
        self.max_depth = 50
        self.background_color = (0.70, 0.80, 1.00)
        self.seed = int(seed)
        self.use_stackless_traversal = USE_STACKLESS_TRAVERSAL
        # integrator whose samples the accumulator holds (checkpoint state):
        # render_sample() and render() use the megakernel
        self._integrator_label = 'megakernel'
        # periodic checkpoints during render(): every `checkpoint_every` progress chunks
        self.checkpoint_path = None
        self.checkpoint_every = 1
        self._resume_state = None
        self._resume_tiles = None  # load_checkpoint(): the tile buffers of an adaptive render's checkpoint
        # adaptive sampling (render_adaptive): per-pixel stats, tile buffers, parameters, per-pass log
        self.stats = None
        self._tiles = None
        self._adaptive = None
        self.adaptive_passes = []
        # denoise(): the filtered image, the variance it claims, the seconds it took (derived: not checkpointed)
        self.denoised = None
        self.denoised_var = None
        self.denoise_seconds = None
        # guides() / guides_ids(): (_guide_key() they were traced for, guide image, id image or None), and the
        # seconds the trace took
        self._guide_cache = (None, None, None)
        self.guide_trace_seconds = None
        # reproject_history(): the (accum, stats) pair it writes into next, swapped with the live pair on each call
        self._history_spare = None
        # render_validated(): its fresh pair, its output pair (swapped with the live pair on each call) and the
        # weight image, and the kept fraction of the history it last returned
        self._validate_scratch = None
        self.last_history_kept = None
        # update_primitives(): bumped on every scene update; part of the guides' cache key
        self.scene_revision = 0
        # rebuild_bvh() and update_primitives(rebuild=...): rebuilds done, and the (mean, max) growth 'auto' last read
        self.bvh_rebuilds = 0
        self.last_tree_growth = None
        # motion blur (ptmi.pose): the shutter interval (None: off), the samples per pose, set_motion's displacements
        # of quads and triangles, and (scene_revision, motion edits, shutter) the resident tracks were made for
        self.shutter = shutter
        self.slice_spp = slice_spp
        self._motion = {'quads': {}, 'triangles': {}}
        self._motion_edits = 0
        self._tracks_key = None
        self._bodies = []  # set_bodies' rigid bodies (ptmi.rigid)
        # launches per progress report: one launch renders many samples (path regeneration)
        self.samples_per_launch = int(samples_per_launch)
        device.require_gpu()
        # renderer.py:78-80: Perlin tables from a perlin() made after the scene
        perlin = core.perlin()
        t0 = time.time()
        (geom, mats, spheres, qgeom, qmats, quads, tgeom, tmats, tris, img_reg,
         img_list) = scene_compiler.compile_scene(world)
        # the primitive objects in compile order and the image registry: update_primitives checks replacements by them
        self._prims = {'spheres': spheres, 'quads': quads, 'triangles': tris}
        self._img_reg = img_reg
        self.timing['scene_compile'] = time.time() - t0
        t0 = time.time()
        bvh = bvh_mod.compile_bvh(world, spheres, quads, tris)
        self.timing['bvh_compile'] = self.timing['bvh_flatten'] = time.time() - t0
        t0 = time.time()
        images = [scene_compiler.image_u8(t) for t in img_list]
        self.arrays = SceneArrays.from_compiled(geom, mats, qgeom, qmats, tgeom, tmats, bvh, perlin.tables(),
                                                images)
        self.dscene = device.DeviceScene.from_arrays(self.arrays, device_id)
        self.integrator = device.Integrator(self.dscene)
        self.accum = torch.zeros((self.cam.img_height, self.cam.img_width, 3), dtype=torch.float32,
                                 device=self.dscene.device)
        self._upload_camera()
        self.timing['gpu_upload'] = self.timing['camera_upload'] = time.time() - t0
        self.timing['total_setup'] = time.time() - t_setup

    # ------------------------------------------------------------------ state
    def _upload_camera(self):
        """renderer.py:230-247: camera + background + max_depth as f32/i32."""
        W, H = self.cam.img_width, self.cam.img_height
        self.frame = device.make_frame(self.cam, self.background_color, self.max_depth, self.seed, W, H,
                                       traversal='stackless' if self.use_stackless_traversal else 'stack')
        if tuple(self.accum.shape[:2]) != (H, W):
            self.accum = torch.zeros((H, W, 3), dtype=torch.float32, device=self.dscene.device)

    def _upload_camera_to_gpu(self):
        self._upload_camera()

    @property
    def num_spheres(self):
        return self.arrays.num_spheres

    @property
    def num_bvh_nodes(self):
        return self.arrays.num_bvh_nodes

    def clear_accumulation_buffer(self):
        self.integrator.clear(self.frame, self.accum)

    # ---------------------------------------------------------------- renders
    def render_sample(self, sample: int):
        """One sample of every pixel (renderer.py:551-556): sample index
        ``sample`` of the counter-based stream, megakernel."""
        self._integrator_label = 'megakernel'
        self._trace(self.integrator.render_mk, self.accum, begin=int(sample), count=1)

    # ------------------------------------------------------------ motion blur
    def set_motion(self, spheres=None, quads=None, triangles=None):
        """Give primitives a linear motion for ``shutter`` renders (DESIGN.md
        §24). Each argument maps a reference primitive index (as in
        ``primitives``) to a ``vec3`` displacement over unit time; None as a
        value removes the motion. For a sphere the displacement replaces its
        ``center.direction`` (``primitives`` then holds a copy of the object);
        quads and triangles keep theirs in the renderer. The resident scene,
        which is the rest pose, does not change, and neither does the image."""
        given = {'spheres': spheres or {}, 'quads': quads or {}, 'triangles': triangles or {}}
        for name, new in given.items():
            have = self._prims[name]
            for i, d in new.items():
                if not isinstance(i, (int, np.integer)) or not 0 <= i < len(have):
                    raise ValueError(f'{name}: no primitive {i!r} (the scene has {len(have)})')
                if d is not None and not (isinstance(d, core.vec3) and all(np.isfinite(d.to_list()))):
                    raise ValueError(f'{name}[{i}]: the displacement must be a finite vec3 or None')
        for i, d in given['spheres'].items():
            obj = copy.copy(self._prims['spheres'][i])
            obj.center = core._center(obj.center.origin, d.copy() if d is not None else core.vec3(0, 0, 0))
            self._prims['spheres'][i] = obj
        for name in ('quads', 'triangles'):
            for i, d in given[name].items():
                if d is None:
                    self._motion[name].pop(int(i), None)
                else:
                    self._motion[name][int(i)] = d.copy()
        self._motion_edits += 1

    def _linearly_moving(self):
        """{kind: the reference indices with a linear motion}: set_motion's entries and the moving spheres."""
        tracks = pose_mod.tracks_of(self._prims, self._motion)
        return {name: set(tracks[name]) for name in tracks}

    def set_bodies(self, bodies):
        """Make groups of primitives rigid bodies for ``shutter`` renders
        (ptmi.rigid): ``bodies`` is a list of ``rigid.Body``, at
        most ``rigid.MAX_BODIES``, and replaces all earlier ones; ``[]`` clears
        them. A primitive that is in two bodies, that is both in a body and
        linearly moving (a ``set_motion`` entry, or a sphere whose
        ``center.direction`` is not zero), or that the scene does not have is a
        ValueError. The resident scene, which is the rest pose, does not
        change, and neither does an image without a shutter. Frame ``k`` of an
        animation is ``shutter = (k * dt, k * dt + exposure)`` and a render:
        ``shutter=(t, t)`` is the still pose at ``t``."""
        bodies = list(bodies)
        members = rigid_mod.members_of(bodies)
        moving = self._linearly_moving()
        for name, have in self._prims.items():
            for i in members[name]:
                if i >= len(have):
                    raise ValueError(f'{name}: no primitive {i!r} (the scene has {len(have)})')
                if i in moving[name]:
                    raise ValueError(f'{name}[{i}] is in a body and moves linearly')
        self._bodies = bodies
        self._motion_edits += 1

    def _ensure_tracks(self):
        """The resident tracks of the scene as it is now: made on the first use, remade when the scene or the
        motion has changed since (or the scene dropped them); when only the shutter has, the resident tracks get
        the new range (DeviceScene.set_t_range: nothing is uploaded, which is what an animation's frame costs)."""
        shutter, self.slice_spp = pose_mod.check_shutter(self.shutter, self.slice_spp)
        key = (self.scene_revision, self._motion_edits, shutter)
        if self._tracks_key is not None and key[:2] == self._tracks_key[:2] and self.dscene._tracks is not None:
            if key != self._tracks_key:
                torch.cuda.synchronize(self.dscene.device)  # set_t_range poses the scene: no render in flight
                self.dscene.set_t_range(shutter)
                self._tracks_key = key
        else:
            torch.cuda.synchronize(self.dscene.device)  # set_tracks poses the scene: no render in flight
            tracks = pose_mod.tracks_of(self._prims, self._motion)
            rigid = (self._bodies, rigid_mod.body_records(self._bodies, self._prims)) if self._bodies else None
            if rigid is not None:  # a set_motion after set_bodies may have named a body's primitive
                members = rigid_mod.members_of(self._bodies)
                for name in tracks:
                    both = sorted(set(tracks[name]) & set(members[name]))
                    if both:
                        raise ValueError(f'{name}[{both[0]}] is in a body and moves linearly')
            self.dscene.set_tracks(*pose_mod.track_records(tracks), t_range=shutter, rigid=rigid)
            self._tracks_key = key
        return shutter

    def _trace(self, render_fn, *buffers, begin, count, **kwargs):
        """``render_fn(frame, *buffers, begin, count, **kwargs)``, or with a shutter the same samples through
        Integrator.render_posed, slice by slice, and the device back at the rest scene whatever happens."""
        if self.shutter is None:
            return render_fn(self.frame, *buffers, begin, count, **kwargs)
        shutter = self._ensure_tracks()
        try:
            self.integrator.render_posed(render_fn, self.frame, begin, count, self.slice_spp, shutter, *buffers,
                                         **kwargs)
        finally:
            self.integrator.unpose()

    def _drop_denoised(self):
        self.denoised = self.denoised_var = self.denoise_seconds = None

    def _restart_image(self, adaptive=None):
        """The image starts over: the sample count and times, the accumulator,
        the counters and, with ``adaptive`` (by default: if there are stats),
        the error estimates, the tile states and ``denoised``."""
        self.current_sample = 0
        self.sample_times = []
        self.clear_accumulation_buffer()
        if adaptive or (adaptive is None and self.stats is not None):
            self._adaptive_reset()
        self.integrator.reset_counters()

    def _begin_render(self, warm_up, resume, what, adaptive):
        """The prologue of a render: the state of a loaded checkpoint checked
        and kept (``resume``), or one warm-up sample rendered and the image
        started over (renderer.py:381-385); the counters reset either way."""
        t0 = time.time()
        if resume:
            if self._resume_state is None:
                raise ValueError(f'{what}(resume=True) needs load_checkpoint() first')
            self._check_resume_state()
            self.integrator.reset_counters()
        else:
            warm_up(self.frame, self.accum, 0, 1)
            torch.cuda.synchronize(self.dscene.device)
            times = self.sample_times
            self._restart_image(adaptive)
            self.sample_times = times  # like the reference's, a render adds to the times of the renders before it
        self._resume_state = None
        torch.cuda.synchronize(self.dscene.device)
        self.timing['kernel_warmup'] = time.time() - t0

    def _run(self, render_fn, label, resume=False):
        self._integrator_label = label
        self._upload_camera()
        spp = int(self.cam.samples_per_pixel)
        self._begin_render(render_fn, resume, 'render', adaptive=False)
        print(f'\n{self.__class__.__name__} ({label})')
        print(f'Resolution: {self.cam.img_width}x{self.cam.img_height} | Samples: {spp} | Depth: {self.max_depth}')
        print(f'Spheres: {self.num_spheres} | BVH Nodes: {self.num_bvh_nodes}')
        per = self.samples_per_launch or max(1, spp // 20)  # ~20 progress reports, like renderer.py:402
        self.render_start_time = time.time()
        done = self.current_sample
        while done < spp:
            n = min(per, spp - done)
            t = time.time()
            self._trace(render_fn, self.accum, begin=done, count=n)
            torch.cuda.synchronize(self.dscene.device)
            dt = time.time() - t
            self.sample_times += [dt / n] * n
            done += n
            self.current_sample = done
            pps = self.cam.img_width * self.cam.img_height * n / dt if dt > 0 else 0.0
            print(f'{done:5d}/{spp} ({100.0 * done / spp:5.1f}%) | {dt * 1e3 / n:7.2f} ms/sample | '
                  f'{pps / 1e6:8.2f} Msamples/s')
            if self.checkpoint_path and done < spp and (done // per) % max(1, self.checkpoint_every) == 0:
                self.save_checkpoint(self.checkpoint_path)
        self.write_image()
        self.print_statistics()

    def render(self, enable_preview: bool = True, resume: bool = False):
        """Megakernel render of cam.samples_per_pixel samples (renderer.py:361-434).
        resume=True continues from a load_checkpoint() state."""
        self._run(self.integrator.render_mk, 'megakernel', resume)

    def render_wavefront(self, enable_preview: bool = True, resume: bool = False):
        """Wavefront render (renderer.py:249-359)."""
        self._run(self.integrator.render_wf, 'wavefront', resume)

    # --------------------------------------------------------------- adaptive
    def _adaptive_reset(self):
        """Zeroed stats and all tiles active, for the current frame."""
        H, W = self.cam.img_height, self.cam.img_width
        if self.stats is None or tuple(self.stats.shape[:2]) != (H, W):
            self.stats = self.integrator.new_stats(self.frame)
        else:
            self.integrator.clear_stats(self.frame, self.stats)
        self._tiles = self.integrator.new_tiles(self.frame)
        self._drop_denoised()  # of the render this one replaces

    def render_adaptive(self, target_error, pass_spp=None, min_spp=16, max_spp=None, integrator='megakernel',
                        resume=False, enable_preview: bool = True, tiles=None):
        """Adaptive render (no counterpart in the reference, which always runs
        cam.samples_per_pixel samples of every pixel). Pass k renders samples
        [k * pass_spp, (k + 1) * pass_spp) of the tiles still active, through
        the stats path (per-pixel {n, mean, M2} of the sample luminance), then
        updates the tiles: a tile is done once it has min_spp samples and its
        error (the mean relative standard error of its pixels' luminance) is
        at most target_error, or at max_spp samples (default
        cam.samples_per_pixel). Stops when no tile is active. A tile whose
        error is NaN (a NaN sample) is done. ``tiles``: whether a pass traces
        the active tiles only. None is each integrator's default: the
        megakernel lists, integrator='wavefront' renders the whole frame every
        pass and only its stop is adaptive. integrator='wavefront', tiles=True
        passes the active list to the wavefront once fewer than all tiles are
        active (Integrator.render_wf_stats, include/ptmi_wf_tiles.h); the
        megakernel always lists, so tiles=False with it is a ValueError.
        Single device only (band_stride == 1). The image divides each pixel by
        its own sample count. resume=True continues a load_checkpoint() state bit-identically."""
        if integrator not in ('megakernel', 'wavefront'):
            raise ValueError(f'unknown integrator {integrator!r}')
        mk = integrator == 'megakernel'
        if mk and tiles is not None and not tiles:
            raise ValueError("render_adaptive(integrator='megakernel') always traces the listed tiles: tiles=False "
                             'is not available')
        listed = mk or bool(tiles)
        self._integrator_label = 'adaptive-' + integrator
        self._upload_camera()
        if self.frame.band_stride != 1:
            raise ValueError('render_adaptive needs band_stride == 1 (multi-GPU adaptive sampling is out of scope)')
        max_spp = int(self.cam.samples_per_pixel if max_spp is None else max_spp)
        min_spp = int(min_spp)
        pass_spp = int(pass_spp if pass_spp is not None else max(1, min_spp))
        target_error = float(np.float32(target_error))
        if not target_error >= 0.0 or pass_spp < 1 or min_spp < 0 or max_spp < min_spp:
            raise ValueError('render_adaptive needs target_error >= 0, pass_spp >= 1 and 0 <= min_spp <= max_spp')
        self._adaptive = {'target_error': target_error, 'pass_spp': pass_spp, 'min_spp': min_spp, 'max_spp': max_spp,
                          'listed': listed}
        integ = self.integrator
        self._begin_render(integ.render_mk if mk else integ.render_wf, resume, 'render_adaptive', adaptive=True)
        if not resume:
            self.adaptive_passes = []
        tiles = self._tiles
        ntiles = tiles['grid'][0] * tiles['grid'][1]
        print(f'\n{self.__class__.__name__} (adaptive {integrator})')
        print(f'Resolution: {self.cam.img_width}x{self.cam.img_height} | Samples: {min_spp}..{max_spp} in passes of '
              f'{pass_spp} | Target error: {target_error:g} | Depth: {self.max_depth}')
        self.render_start_time = time.time()
        while tiles['n'] > 0 and self.current_sample < max_spp:
            n = min(pass_spp, max_spp - self.current_sample)
            active = tiles['n']
            t = time.time()
            sel = (tiles['list'], active) if listed and active < ntiles else None
            self._trace(integ.render_mk_stats if mk else integ.render_wf_stats, self.accum, self.stats,
                        begin=self.current_sample, count=n, tiles=sel)
            integ.tile_update(self.frame, self.stats, target_error, min_spp, max_spp, tiles)
            torch.cuda.synchronize(self.dscene.device)
            dt = time.time() - t
            self.sample_times += [dt / n] * n
            self.current_sample += n
            traced = (64 * active if listed else self.cam.img_width * self.cam.img_height) * n
            self.adaptive_passes.append({'pass': len(self.adaptive_passes), 'active_tiles': active, 'samples': n,
                                         'traced': traced, 'seconds': dt, 'active_after': tiles['n']})
            print(f'pass {len(self.adaptive_passes):3d} | {self.current_sample:5d}/{max_spp} spp | '
                  f'{active:6d}/{ntiles} tiles | {dt * 1e3:8.2f} ms | {tiles["n"]:6d} tiles left')
            if self.checkpoint_path and tiles['n'] > 0 and self.current_sample < max_spp and \
                    len(self.adaptive_passes) % max(1, self.checkpoint_every) == 0:
                self.save_checkpoint(self.checkpoint_path)
        self.write_image()
        self.print_statistics()

    def noise_map(self):
        """Tile errors of the last tile update, (tiles_y, tiles_x) f32 (+inf before any update)."""
        if self._tiles is None:
            raise ValueError('no adaptive render yet')
        tx, ty = self._tiles['grid']
        return self._tiles['err'].cpu().numpy().reshape(ty, tx)

    def sample_count_map(self):
        """Samples accumulated per pixel through the stats path, (height, width) int32."""
        if self.stats is None:
            raise ValueError('no adaptive render yet')
        return self.stats[..., 0].cpu().numpy().astype(np.int32)

    def _guide_key(self):
        f = self.frame
        cam = tuple(float(v) for k in ('center', 'pixel00', 'delta_u', 'delta_v') for v in getattr(f.cam, k))
        return cam + (int(f.width), int(f.height), int(f.traversal), self.scene_revision)

    def guides(self):
        """First-hit guide buffers of the current camera (Integrator.trace_guides,
        include/ptmi_guide.h): a (height, width, 8) f32 tensor {nx, ny, nz,
        depth, ar, ag, ab, hit}. Traced once per camera and scene and cached;
        one deterministic primary ray per pixel, independent of the samples
        rendered."""
        key, guides, _ = self._cached_guides()
        if guides is None:
            t0 = time.time()
            guides = self.integrator.trace_guides(self.frame)
            torch.cuda.synchronize(self.integrator.scene.device)
            self.guide_trace_seconds = time.time() - t0
            self._guide_cache = (key, guides, None)
        return guides

    def _cached_guides(self):
        """The cache entry (key, guides, ids) if it is of the current camera and scene, else (key, None, None)."""
        key = self._guide_key()
        return self._guide_cache if self._guide_cache[0] == key else (key, None, None)

    def guides_ids(self):
        """``(guides, ids)`` of the current camera (Integrator.trace_guides_ids,
        include/ptmi_motion.h): the guides of ``guides()`` and an (height,
        width) int32 tensor naming the primitive each pixel sees (``type << 28
        | device primitive index``, -1 where no surface shows). Traced once per
        camera and scene and cached like ``guides()``, whose tensor it fills
        or reuses."""
        key, have, ids = self._cached_guides()
        if ids is None:
            ids = torch.empty((int(self.frame.height), int(self.frame.width)), dtype=torch.int32,
                              device=self.integrator.scene.device)
            t0 = time.time()
            out = (have if have is not None else torch.empty(tuple(ids.shape) + (8,), dtype=torch.float32,
                                                             device=ids.device), ids)
            self._guide_cache = (key,) + self.integrator.trace_guides_ids(self.frame, out=out)
            torch.cuda.synchronize(self.integrator.scene.device)
            if have is None:
                self.guide_trace_seconds = time.time() - t0
        return self._guide_cache[1:]

    def guide_maps(self):
        """The guides as numpy AOVs: {'normal': (H, W, 3), 'depth': (H, W),
        'albedo': (H, W, 3), 'hit': (H, W) bool}; depth is 1e10 where hit is False."""
        g = self.guides().cpu().numpy()
        return {'normal': g[..., 0:3].copy(), 'depth': g[..., 3].copy(), 'albedo': g[..., 4:7].copy(),
                'hit': g[..., 7] != 0}

    # ----------------------------------------------------------- scene updates
    @property
    def primitives(self):
        """The scene's primitive objects in compile order, {'spheres': [...],
        'quads': [...], 'triangles': [...]}: the indices update_primitives takes."""
        return self._prims

    _REBUILD = 'for any other edit build a new MI355XRenderer from the edited world'

    def update_primitives(self, spheres=None, quads=None, triangles=None, keep_history=False, rebuild=False,
                          rebuild_growth=None, builder='host', **params):
        """Move primitives of the resident scene and refit its BVH on the device
        (DeviceScene.update_primitives, include/ptmi_update.h).
        Each argument maps a reference primitive index (the primitive's place
        in ``compile_scene``'s sphere, quad or triangle list) to the new
        ``Sphere`` / ``quad`` / ``triangle`` object. Only geometry changes:
        the object must be of the list's kind and compile to the material
        record the primitive has (a new material is ``update_materials``');
        counts, order, media and the BVH topology stay (a refit tree traverses
        slower the further objects scatter). Anything else is a ValueError:
        that path is a new renderer.

        The image starts over: the accumulator is cleared, the adaptive state
        is reset as for a new adaptive render, ``denoised`` and the
        reprojection spare pair are dropped, and the guides are retraced on
        their next use. ``arrays`` is afterwards what the device holds, with
        the geometry arrays of a full compile of the edited world.

        ``keep_history=True`` (a stats render is needed, a ValueError
        otherwise) carries the image across the update instead
        (include/ptmi_motion.h): the guides, the id image and a
        copy of the primitive rows are taken before the update, the guides and
        ids are retraced after it, and ``reproject_history`` moves ``accum``
        and ``stats`` to where every surface point went, with ``params`` as
        its parameters. The accumulator is not cleared and ``current_sample``
        stays; the tile states start over and ``denoised`` is dropped. Returns
        the fraction of pixels with history (None without keep_history).

        ``rebuild``: False, the default, refits only and
        launches nothing else. True rebuilds the BVH in place after the refit
        (``rebuild_bvh``). 'auto' reads the refit tree's mean box growth
        (``tree_growth``, kept as ``last_tree_growth``) and rebuilds if it
        exceeds ``rebuild_growth`` (default ``ptmi.tree.REBUILD_GROWTH``; a
        ValueError where neither is set). The default is the growth at which
        a rebuild pays for itself within one 64-spp 800x800 step, where the
        refit tree already renders at about half the rebuilt rate: a
        loop that renders several steps per update should pass a lower one
        (DESIGN.md §20 has the sweep). A rebuild bumps ``scene_revision``
        once more and does to the image what the update does: with
        ``keep_history`` the history's ids and primitive rows are carried to
        the new device order before the reprojection. Reference indices do
        not change across a rebuild; the device rows in ``guides_ids()`` do.
        ``builder`` is ``rebuild_bvh``'s: with 'device' the default threshold
        of 'auto' is ``ptmi.build.REBUILD_GROWTH_DEVICE``."""
        threshold = self._rebuild_threshold(rebuild, rebuild_growth, builder)
        history = self._take_history(keep_history, params)
        self._apply_update(spheres, quads, triangles)
        maps = self._rebuild_scene(builder) if self._wants_rebuild(rebuild, threshold) else None
        return self._after_scene_change(history, maps, params)

    def _take_history(self, keep_history, params):
        """The _History of the image before a scene change that keeps it, else None (and then no ``params``)."""
        if keep_history:
            if self.stats is None:
                raise ValueError('keep_history=True needs stats: render through the stats path (render_adaptive) first')
            return _History(self.frame.cam, *self.guides_ids(), self.dscene.primitive_rows())
        if params:
            raise ValueError(f'{sorted(params)} are reprojection parameters: they need keep_history=True')
        return None

    def _after_scene_change(self, history, maps, params):
        """What becomes of the image after an update, a rebuild (``maps``: its
        row maps, else None) or both: reprojected from ``history``, or started over."""
        if history is not None:
            if maps is not None:
                history = self._history_across_rebuild(history, maps)
            return self._reproject_from(history, **params)
        self._restart_image()
        self.adaptive_passes = []
        self._history_spare = None
        self._guide_cache = (None, None, None)

    # ------------------------------------------------- tree quality and rebuild
    def tree_growth(self):
        """``(mean, max)`` growth of the BVH's internal boxes since the tree was
        built or last rebuilt (DeviceScene.tree_growth):
        (1.0, 1.0) until an update moves something."""
        return self.dscene.tree_growth()

    @staticmethod
    def _rebuild_threshold(rebuild, rebuild_growth, builder='host'):
        """update_primitives' ``rebuild``, ``rebuild_growth`` and ``builder`` checked: the growth
        'auto' rebuilds above, else None."""
        if builder not in ('host', 'device'):
            raise ValueError(f"builder must be 'host' or 'device', not {builder!r}")
        if not (rebuild is True or rebuild is False or rebuild == 'auto'):
            raise ValueError(f"rebuild must be False, True or 'auto', not {rebuild!r}")
        if rebuild != 'auto':
            if rebuild_growth is not None:
                raise ValueError("rebuild_growth is the threshold of rebuild='auto'")
            return None
        if rebuild_growth is None:
            rebuild_growth = build_mod.REBUILD_GROWTH_DEVICE if builder == 'device' else tree_mod.REBUILD_GROWTH
        if rebuild_growth is None:
            raise ValueError("rebuild='auto' needs rebuild_growth=: no default has been measured "
                             f"(ptmi.{'build.REBUILD_GROWTH_DEVICE' if builder == 'device' else 'tree.REBUILD_GROWTH'})")
        rebuild_growth = float(rebuild_growth)
        if not rebuild_growth >= 1.0:
            raise ValueError('rebuild_growth is a mean box-area growth: at least 1.0')
        return rebuild_growth

    def _wants_rebuild(self, rebuild, threshold):
        """After the refit: rebuild now? 'auto' reads the tree's mean growth (one launch, one 16-byte readback)."""
        if rebuild == 'auto':
            self.last_tree_growth = self.dscene.tree_growth()
            return self.last_tree_growth[0] > threshold
        return bool(rebuild)

    def _rebuild_scene(self, builder='host'):
        """DeviceScene.rebuild with no render in flight; bumps ``scene_revision``. Returns its row maps."""
        torch.cuda.synchronize(self.dscene.device)
        maps = self.dscene.rebuild(builder=builder)
        self.arrays = self.dscene.arrays
        self.scene_revision += 1
        self.bvh_rebuilds += 1
        return maps

    def _history_across_rebuild(self, history, maps):
        """A history taken before a rebuild in the device order after it: its ids
        remapped (ptmi_ids_remap) and its primitive rows permuted."""
        return _History(history.camera, history.guides, self.dscene.remap_ids(history.ids, maps),
                        self.dscene.permute_rows(history.rows, maps))

    def rebuild_bvh(self, keep_history=False, builder='host', **params):
        """Rebuild the resident scene's BVH in place (DeviceScene.rebuild,
        DESIGN.md §20): what a new renderer of the edited world would build,
        without a new renderer. The device tensors, their pointers, this
        renderer and its integrator stay; ``scene_revision`` is bumped and
        ``bvh_rebuilds`` counted. The image is treated as by
        ``update_primitives``: started over, or with ``keep_history=True``
        reprojected (``params`` as there; the history's ids and rows are
        carried to the new device order first). The reference indices that
        ``update_primitives`` and ``primitives`` take do not change; the
        device rows in ``guides_ids()``'s id image do. Returns the fraction of
        pixels with history (None without keep_history). ``builder='device'``
        builds and packs the tree on the device (DeviceScene.rebuild, DESIGN.md
        §23): the same tensors, maps and images byte for byte;
        ``dscene.last_rebuild`` says which path ran."""
        self._rebuild_threshold(False, None, builder)
        history = self._take_history(keep_history, params)
        return self._after_scene_change(history, self._rebuild_scene(builder), params)

    # ------------------------------------------------------------ material edits
    _MATERIAL_KINDS = ('lambertian', 'metal', 'dielectric', 'diffuse_light')
    # per primitive class: the attribute that holds its material, and a reference point (scene_compiler's)
    _PRIM_PARTS = {'Sphere': ('material', lambda o: o.center.at(0.0)), 'quad': ('mat', lambda o: o.Q),
                   'triangle': ('mat', lambda o: o.v0)}

    def update_materials(self, spheres=None, quads=None, triangles=None, media=None, keep_history=False, **params):
        """Edit materials of the resident scene on the device
        (DeviceScene.update_materials, include/ptmi_material.h)
        instead of building a new renderer. ``spheres``, ``quads`` and
        ``triangles`` map a reference primitive index (as in ``primitives``) to
        the primitive's new material object: a ``lambertian`` (solid, checker,
        noise or image texture), ``metal``, ``dielectric`` or
        ``diffuse_light``. Its record is the scene compiler's own, so the
        material arrays are afterwards those of a full compile of the edited
        world. An ``image_texture`` must be one the scene was compiled with
        (its texels are resident); any other is a ValueError that names the
        rebuild path. ``primitives`` then holds copies of the objects with the
        new materials.

        Whether a primitive is the boundary of a constant medium is fixed, and
        its medium fields are kept. ``media`` maps ``(kind, index)``, e.g.
        ``('spheres', 3)``, of a primitive that is such a boundary to
        ``(density, albedo)``, the medium's new density and the new albedo of
        its phase function (three floats); for any other primitive it is a
        ValueError. Counts, geometry and the BVH do not change.

        The image is treated as by ``update_primitives``: by default it starts
        over and the guides are retraced on their next use. With
        ``keep_history=True`` (a stats render is needed) it is reprojected
        through ``reproject_history`` with ``params``: the primitives have not
        moved, and a surface whose guide albedo changed by more than
        ``sigma_a`` loses its history there. The light that an edit changes on
        other surfaces (a dimmed lamp, a recoloured wall's bounce) lags in the
        kept history until ``render_validated`` has judged it.
        Returns the fraction of pixels with history (None without
        keep_history)."""
        history = self._take_history(keep_history, params)
        self._apply_materials(spheres, quads, triangles, media)
        return self._after_scene_change(history, None, params)

    def _apply_materials(self, spheres, quads, triangles, media):
        """update_materials' checks and the edit itself, up to the bumped
        ``scene_revision``; what becomes of the image is the caller's."""
        given = {k.name: dict(new or {}) for k, new in zip(STORAGE, (spheres, quads, triangles))}
        media = dict(media or {})
        for key in media:
            if not (isinstance(key, tuple) and len(key) == 2 and key[0] in given):
                raise ValueError(f'media: {key!r} is not (kind, index) with kind one of {sorted(given)}')
        args, objects = [], {}
        for k in STORAGE:
            name, have, mats = k.name, self._prims[k.name], getattr(self.arrays, k.materials)
            attr, get_ref = self._PRIM_PARTS[k.class_name]
            fog = {i: v for (kind, i), v in media.items() if kind == name}
            records, order = [], sorted(set(given[name]) | set(fog))
            for i in order:
                if not isinstance(i, (int, np.integer)) or not 0 <= i < len(have):
                    raise ValueError(f'{name}: no primitive {i!r} (the scene has {len(have)}); {self._REBUILD}')
                rec = {key: mats[key][i] for key in mats}  # the current record; the medium fields stay
                if i in given[name]:
                    mat = given[name][i]
                    if type(mat).__name__ not in self._MATERIAL_KINDS:
                        raise ValueError(f'{name}[{i}]: {type(mat).__name__} is not a material '
                                         f'({", ".join(self._MATERIAL_KINDS)})')
                    tex = getattr(mat, 'tex', None)
                    if type(tex).__name__ == 'image_texture' and id(tex) not in self._img_reg:
                        raise ValueError(f'{name}[{i}]: the image texture is not one the scene was compiled with, '
                                         f'so its texels are not resident; {self._REBUILD}')
                    rec.update(scene_compiler._material_row(mat, get_ref(have[i]), self._img_reg))
                    objects[name, i] = copy.copy(have[i])
                    setattr(objects[name, i], attr, mat)
                if i in fog:
                    if not rec['is_constant_medium']:
                        raise ValueError(f'media: {name}[{i}] is not the boundary of a constant medium; which '
                                         f'primitives are is fixed, {self._REBUILD}')
                    density, albedo = fog[i]
                    albedo = [albedo.x, albedo.y, albedo.z] if hasattr(albedo, 'x') else [float(c) for c in albedo]
                    if len(albedo) != 3:
                        raise ValueError(f'media: {name}[{i}]: the albedo must be three floats')
                    rec.update(medium_density=float(density), medium_albedo=albedo)
                records.append(rec)
            args.append((np.asarray(order, np.int64), scene_compiler.material_rows(records)) if order else None)
        torch.cuda.synchronize(self.dscene.device)  # no render of the scene in flight on any stream (overlapped traces)
        self.dscene.update_materials(*args)
        for (name, i), obj in objects.items():
            self._prims[name][i] = obj
        self.arrays = self.dscene.arrays
        self.scene_revision += 1

    def _apply_update(self, spheres, quads, triangles):
        """update_primitives' checks and the update itself, up to the bumped
        ``scene_revision``; what becomes of the image is the caller's."""
        getters = {'Sphere': (lambda o: o.material, lambda o: o.center.at(0.0)),  # the material, a reference point
                   'quad': (lambda o: o.mat, lambda o: o.Q), 'triangle': (lambda o: o.mat, lambda o: o.v0)}
        given = {k.name: new or {} for k, new in zip(STORAGE, (spheres, quads, triangles))}
        for k in STORAGE:
            name, kind, new, (get_mat, get_ref) = k.name, k.class_name, given[k.name], getters[k.class_name]
            mats, have = getattr(self.arrays, k.materials), self._prims[name]
            for i, obj in new.items():
                if not isinstance(i, (int, np.integer)) or not 0 <= i < len(have):
                    raise ValueError(f'{name}: no primitive {i!r} (the scene has {len(have)}); {self._REBUILD}')
                if type(obj).__name__ != kind:
                    raise ValueError(f'{name}[{i}]: a {type(obj).__name__} cannot replace a {kind}; {self._REBUILD}')
                row = scene_compiler._material_row(get_mat(obj), get_ref(obj), self._img_reg)
                for key, v in row.items():
                    if np.asarray(v, mats[key].dtype).tobytes() != mats[key][i].tobytes():
                        raise ValueError(f'{name}[{i}]: the new object changes {key}; materials are '
                                         f'update_materials\' to edit, {self._REBUILD}')
        order = {name: sorted(new) for name, new in given.items()}
        records = scene_compiler.update_records(*([given[k.name][i] for i in order[k.name]] for k in STORAGE))
        args = [(np.asarray(order[k.name], np.int64), rows, build) if order[k.name] else None
                for k, (rows, build) in zip(STORAGE, records)]
        torch.cuda.synchronize(self.dscene.device)  # no render of the scene in flight on any stream (overlapped traces)
        self.dscene.update_primitives(*args)
        for name, new in given.items():
            for i, obj in new.items():
                self._prims[name][i] = obj
        self.arrays = self.dscene.arrays
        self.scene_revision += 1

    def reproject_history(self, prev_camera, prev_guides, again=False, prev_ids=None, prev_rows=None, match_ids=True,
                          **params):
        """Carry ``accum`` and ``stats`` of a stats render from ``prev_camera``
        (its camera-upload dict or ptmi_camera) with the guides ``prev_guides``
        it had to the current camera (Integrator.reproject,
        include/ptmi_temporal.h; ``params`` are its max_history, sigma_z,
        normal_min and sigma_a). The guides of the current camera are traced
        or taken from the cache (``prev_guides`` may be that same tensor: the
        camera has not moved); the result is written into spare tensors that
        are then swapped in, the tile states start over and ``denoised`` is
        dropped. Returns the fraction of pixels with history.

        ``again=True``, for a camera that moved on with no sample rendered
        since the last call: the history that call reprojected (kept as the
        spare pair; ``prev_camera`` and ``prev_guides`` are still its own) is
        reprojected to the current camera and replaces that call's result, so
        a drag of many steps resamples and caps the rendered history once, not
        once per step. Derived state: not checkpointed.

        ``prev_ids`` and ``prev_rows``, both or neither (one alone is a
        ValueError): the id image the history's frame had (``guides_ids()``)
        and the primitive rows of its scene (``DeviceScene.primitive_rows()``),
        for a scene updated since. The reprojection is then the motion-aware
        one (Integrator.reproject_moved, include/ptmi_motion.h, DESIGN.md
        §18), with ``match_ids`` as its flag."""
        if self.stats is None:
            raise ValueError('no stats: render through the stats path (render_adaptive) first')
        if (prev_ids is None) != (prev_rows is None):
            raise ValueError('prev_ids and prev_rows go together: the id image and the primitive rows of the '
                             'history\'s frame')
        return self._reproject_from(_History(prev_camera, prev_guides, prev_ids, prev_rows), again, match_ids,
                                    **params)

    def _reproject_from(self, history, again=False, match_ids=True, **params):
        """reproject_history from the history's camera, guides and, if it has rows, ids and rows."""
        cam, integ = self.frame.cam, self.integrator
        if history.rows is None:
            guides = self.guides()

            def reproject(accum, stats, out):
                return integ.reproject(cam, history.camera, guides, history.guides, accum, stats, out=out, **params)
        else:
            guides, ids = self.guides_ids()

            def reproject(accum, stats, out):
                return integ.reproject_moved(cam, history.camera, guides, history.guides, ids, history.ids,
                                             history.rows, accum, stats, match_ids=match_ids, out=out, **params)
        spare = self._history_spare
        if spare is not None and tuple(spare[0].shape) != tuple(self.accum.shape):
            spare = None
        if again:
            if spare is None:
                raise ValueError('again=True needs an earlier reproject_history() of this image size')
            reproject(spare[0], spare[1], (self.accum, self.stats))
        else:
            if spare is None:
                spare = (torch.empty_like(self.accum), torch.empty_like(self.stats))
            out = reproject(self.accum, self.stats, spare)
            self._history_spare = (self.accum, self.stats)
            self.accum, self.stats = out
        self._tiles = self.integrator.new_tiles(self.frame)
        self._drop_denoised()
        return int((self.stats[..., 0] > 0).sum().item()) / (self.stats.shape[0] * self.stats.shape[1])

    def render_validated(self, spp, integrator='megakernel', **params):
        """Render ``spp`` fresh samples and let them judge the carried history
        (Integrator.validate_history, include/ptmi_validate.h):
        the call for the step after ``update_primitives(keep_history=True)``
        or ``reproject_history``. The samples, from ``next_sample_index`` (a
        viewer's) or ``current_sample`` on, go through the stats path of
        ``integrator`` ('megakernel' or 'wavefront') into a cleared scratch
        pair; ``accum`` and ``stats`` are validated against that pair and
        merged with it into a second scratch pair, which is then swapped in.
        Where a window of pixels says the light has changed, the history is
        dropped and the pixel starts over from the fresh samples; elsewhere the
        result is what rendering ``spp`` samples on top of the history gives,
        up to the rounding of a merge of two Welford states. ``params`` are
        ``radius``, ``k_lo`` and ``k_hi``.

        ``current_sample`` advances by ``spp``, the tile states start over and
        ``denoised`` is dropped. Returns the kept fraction of the history,
        sum(n_v) / sum(n_h) over the image (1.0 where there was none), also
        kept as ``last_history_kept``. Needs stats, and ``spp >= 2``: one
        sample has no variance to judge by (ValueError). The scratch pairs are
        the renderer's, made once per image size, apart from the spare pair of
        ``reproject_history``. Derived state: not checkpointed. Single device,
        whole frames."""
        if integrator not in ('megakernel', 'wavefront'):
            raise ValueError(f'unknown integrator {integrator!r}')
        if self.stats is None:
            raise ValueError('render_validated needs stats: render through the stats path (render_adaptive) first')
        spp = int(spp)
        if spp < 2:
            raise ValueError('render_validated needs spp >= 2: a pixel with one fresh sample has no variance to '
                             'judge its history by')
        if self.frame.band_stride != 1:
            raise ValueError('render_validated needs band_stride == 1 (banded frames are out of scope)')
        integ = self.integrator
        sc = self._validate_scratch
        if sc is None or tuple(sc['fresh'][0].shape) != tuple(self.accum.shape):
            pair = lambda: (torch.empty_like(self.accum), torch.empty_like(self.stats))  # noqa: E731
            sc = self._validate_scratch = {'fresh': pair(), 'out': pair(),
                                           'weight': torch.empty(tuple(self.stats.shape[:2]), dtype=torch.float32,
                                                                 device=self.stats.device)}
        fresh_accum, fresh_stats = sc['fresh']
        integ.clear(self.frame, fresh_accum)
        integ.clear_stats(self.frame, fresh_stats)
        self._integrator_label = 'adaptive-' + integrator
        begin = getattr(self, 'next_sample_index', self.current_sample)
        t = time.time()
        self._trace(integ.render_mk_stats if integrator == 'megakernel' else integ.render_wf_stats,
                    fresh_accum, fresh_stats, begin=begin, count=spp)
        hist = (self.accum, self.stats)
        out = integ.validate_history(*hist, fresh_accum, fresh_stats, out=sc['out'], weight=sc['weight'], **params)
        # sum(n_v) / sum(n_h): n_v = weight * n_h, whole numbers; a non-finite history pixel counts as empty
        ok = torch.isfinite(hist[0]).all(-1) & torch.isfinite(hist[1][..., :3]).all(-1)
        n_h = torch.where(ok, hist[1][..., 0], torch.zeros_like(sc['weight'])).double()
        n_v = torch.round(sc['weight'].double() * n_h)
        total, kept = float(n_h.sum().item()), float(n_v.sum().item())
        self.accum, self.stats = out
        sc['out'] = hist
        dt = time.time() - t
        self.sample_times += [dt / spp] * spp
        self.current_sample += spp
        self._tiles = integ.new_tiles(self.frame)
        self._drop_denoised()
        self.last_history_kept = kept / total if total > 0 else 1.0
        return self.last_history_kept

    def denoise(self, iterations=5, sigma=4.0, guided=False, **guided_params):
        """Variance-guided a-trous filter of the accumulator by the per-pixel
        error estimates of the stats render that filled it (Integrator.denoise,
        include/ptmi_post.h). Stores ``denoised`` ((height, width, 3) f32
        tensor, linear, already divided by the sample counts) and
        ``denoised_var`` ((height, width): the variance of the mean luminance
        the filter claims) and returns ``denoised``. A uniform render with
        stats is render_adaptive(target_error=0, min_spp=N, max_spp=N). Single
        device: a multi-GPU render gathers the accumulator only, not the stats.

        guided=True: the same with the guides of ``guides()`` as further
        edge-stopping terms (Integrator.denoise_guided, include/ptmi_guide.h);
        ``guided_params`` are its sigma_z, sigma_a, normal_power_log2 and
        demodulate."""
        if not self._is_adaptive():
            raise ValueError('no stats: render through render_adaptive')
        if guided_params and not guided:
            raise ValueError(f'{sorted(guided_params)} need guided=True')
        guides = self.guides() if guided else None  # (its own time is guide_trace_seconds)
        t0 = time.time()
        if guided:
            self.denoised, self.denoised_var = self.integrator.denoise_guided(self.accum, self.stats, guides,
                                                                              iterations, sigma, **guided_params)
        else:
            self.denoised, self.denoised_var = self.integrator.denoise(self.accum, self.stats, iterations, sigma)
        torch.cuda.synchronize(self.integrator.scene.device)
        self.denoise_seconds = time.time() - t0
        return self.denoised

    def _is_adaptive(self):
        return self._integrator_label.startswith('adaptive-') and self.stats is not None

    # ------------------------------------------------------- checkpoint/resume
    # what must match for a checkpoint to continue this render exactly; the
    # integrator too: megakernel and wavefront paths differ (Q1, Q11, Q14), so
    # a render resumed with the other one would match neither uninterrupted render
    _STATE_KEYS = ('integrator', 'seed', 'max_depth', 'background', 'traversal', 'width', 'height', 'camera',
                   'scene')
    # the shutter and the samples per pose: absent from a checkpoint written before there was a shutter, which is
    # one of an unblurred render
    # 'bodies': rigid.digest of set_bodies' bodies under a shutter; absent or '' means no bodies
    _SHUTTER_KEYS = {'shutter': np.zeros(0, np.float64), 'slice_spp': np.int64(0), 'bodies': np.array('')}

    def _render_state(self):
        import hashlib
        lay = self.dscene.layout
        h = hashlib.sha256()
        for a in (lay.nodes, lay.spheres, lay.quads, lay.tris, lay.mats, lay.texels, lay.perlin_vec, lay.perlin_perm):
            h.update(np.ascontiguousarray(a).tobytes())
        f = self.frame
        cam = np.array([list(f.cam.center), list(f.cam.pixel00), list(f.cam.delta_u), list(f.cam.delta_v),
                        list(f.cam.defocus_u), list(f.cam.defocus_v), [f.cam.defocus_angle, 0.0, 0.0]], np.float32)
        return {'integrator': np.array(self._integrator_label), 'seed': np.int64(f.seed), 'max_depth': np.int64(f.max_depth),
                'background': np.array(list(f.bg), np.float32), 'traversal': np.int64(f.traversal),
                'width': np.int64(f.width), 'height': np.int64(f.height), 'camera': cam,
                'scene': np.array(h.hexdigest()), **self._shutter_state()}

    def _shutter_state(self):
        if self.shutter is None:
            return dict(self._SHUTTER_KEYS)
        shutter, slice_spp = pose_mod.check_shutter(self.shutter, self.slice_spp)
        return {'shutter': np.array(shutter, np.float64), 'slice_spp': np.int64(slice_spp),
                'bodies': np.array(rigid_mod.digest(self._bodies) if self._bodies else '')}

    def save_checkpoint(self, path):
        """Write the accumulator and the next sample index (plain arrays, npz)
        to exactly ``path`` (no suffix added). The file is written next to it
        under a temporary name and renamed over it, so a crash mid-save leaves
        the previous checkpoint intact."""
        import tempfile
        torch.cuda.synchronize(self.dscene.device)
        st = self._render_state()
        acc = self.accum.cpu().numpy()
        if self._is_adaptive() and self._adaptive is not None:  # stats, tile state and the adaptive parameters too
            a = self._adaptive
            st.update(stats=self.stats.cpu().numpy(), tile_state=self._tiles['state'].cpu().numpy(),
                      tile_err=self._tiles['err'].cpu().numpy(),
                      adaptive=np.array([a['target_error'], a['pass_spp'], a['min_spp'], a['max_spp'],
                                         float(a['listed'])], np.float64),
                      adaptive_passes=np.array([[q['active_tiles'], q['samples'], q['traced'], q['active_after']]
                                                for q in self.adaptive_passes], np.int64).reshape(-1, 4),
                      adaptive_seconds=np.array([q['seconds'] for q in self.adaptive_passes], np.float64))
        d = os.path.dirname(os.path.abspath(path))
        fd, tmp = tempfile.mkstemp(prefix='.ckpt-', suffix='.npz', dir=d)
        try:
            with os.fdopen(fd, 'wb') as f:
                np.savez(f, accum=acc, next_sample=np.int64(self.current_sample), **st)
            os.replace(tmp, path)
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise

    def load_checkpoint(self, path):
        """Load a save_checkpoint() file into this renderer; render(resume=True)
        then renders samples next_sample .. cam.samples_per_pixel - 1. The
        render state (scene arrays, camera, seed, max_depth, background,
        traversal) is checked when the render resumes, after the
        render-time attributes have been applied."""
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in self._STATE_KEYS if k not in z.files]
            if missing:
                raise ValueError(f'{path} is not a checkpoint of this renderer version (missing {missing})')
            state = {k: z[k].copy() for k in self._STATE_KEYS}
            state.update({k: z[k].copy() if k in z.files else v for k, v in self._SHUTTER_KEYS.items()})
            acc = z['accum'].copy()
            nxt = int(z['next_sample'])
            ad = {k: z[k].copy() for k in ('stats', 'tile_state', 'tile_err', 'adaptive', 'adaptive_passes',
                                           'adaptive_seconds')} if 'adaptive' in z.files else None
        if acc.dtype != np.float32 or acc.ndim != 3 or acc.shape[2] != 3:
            raise ValueError(f'checkpoint accumulator has shape {acc.shape} / {acc.dtype}')
        self.accum = torch.from_numpy(acc).to(self.dscene.device)
        self.current_sample = nxt
        self._resume_state = state
        if ad is not None:  # an adaptive render's checkpoint: render_adaptive(resume=True) continues it
            dev = self.dscene.device
            if ad['stats'].dtype != np.float32 or ad['stats'].shape != acc.shape[:2] + (4,):
                raise ValueError(f'checkpoint stats have shape {ad["stats"].shape} / {ad["stats"].dtype}')
            self.stats = torch.from_numpy(ad['stats']).to(dev)
            ids = np.flatnonzero(ad['tile_state']).astype(np.int32)
            lst = np.zeros(ad['tile_state'].size, np.int32)
            lst[:ids.size] = ids
            if ad['adaptive'].size == 4:  # written before the tiles flag: the integrator's default
                default = str(state['integrator']) == 'adaptive-megakernel'
                ad['adaptive'] = np.append(ad['adaptive'], float(default))
            self._resume_state['adaptive'] = ad['adaptive']
            self._resume_tiles = {'state': torch.from_numpy(ad['tile_state'].astype(np.int32)).to(dev),
                                  'err': torch.from_numpy(ad['tile_err'].astype(np.float32)).to(dev),
                                  'list': torch.from_numpy(lst).to(dev), 'n': int(ids.size)}
            self.adaptive_passes = [{'pass': i, 'active_tiles': int(r[0]), 'samples': int(r[1]), 'traced': int(r[2]),
                                     'seconds': float(sec), 'active_after': int(r[3])}
                                    for i, (r, sec) in enumerate(zip(ad['adaptive_passes'], ad['adaptive_seconds']))]

    def _check_resume_state(self):
        cur = self._render_state()
        for k in self._STATE_KEYS + tuple(self._SHUTTER_KEYS):
            if not np.array_equal(cur[k], self._resume_state[k]):
                raise ValueError(f'checkpoint was written for another render: {k} differs')
        if tuple(self.accum.shape) != (int(cur['height']), int(cur['width']), 3):
            raise ValueError('checkpoint accumulator does not match the image size')
        if self._is_adaptive():  # the adaptive parameters and the tile grid must match too
            a = self._adaptive
            want = np.array([a['target_error'], a['pass_spp'], a['min_spp'], a['max_spp'], float(a['listed'])],
                            np.float64)
            if not np.array_equal(want, self._resume_state.get('adaptive')):
                raise ValueError('checkpoint was written for another render: adaptive differs')
            _, _, tx, ty = self.integrator.tile_grid(self.frame)
            if self._resume_tiles['state'].numel() != tx * ty:
                raise ValueError('checkpoint was written for another render: tile grid differs')
            self._tiles = dict(self._resume_tiles, grid=(tx, ty))

    # ----------------------------------------------------------------- output
    def image_u8(self, sample_count=None, denoised=False):
        if denoised:  # denoise()'s result is already divided by the sample counts
            if self.denoised is None:
                raise ValueError('no denoised image: call denoise() first')
            return self.integrator.tonemap(self.denoised, 1).cpu().numpy()
        if sample_count is None and self._is_adaptive():  # each pixel by its own sample count
            return self.integrator.tonemap(self.accum, stats=self.stats).cpu().numpy()
        spp = self.cam.samples_per_pixel if sample_count is None else sample_count
        return self.integrator.tonemap(self.accum, spp).cpu().numpy()

    def write_image(self):
        """PNG of the tone-mapped accumulator (renderer.py:436-442, preview.py:117-132)."""
        from PIL import Image
        Image.fromarray(self.image_u8(), mode='RGB').save(self.img_path)
        print(f'\nImage saved to {self.img_path}')

    _write_image = write_image

    def write_denoised_image(self, path=None):
        """PNG of the tone-mapped denoise() result, by default next to the
        image as <name>_denoised.png."""
        from PIL import Image
        if path is None:
            root, ext = os.path.splitext(self.img_path)
            path = f'{root}_denoised{ext or ".png"}'
        Image.fromarray(self.image_u8(denoised=True), mode='RGB').save(path)
        print(f'\nDenoised image saved to {path}')
        return path

    def _get_rr_stats(self):
        """Russian-roulette statistics of the last render (renderer.py:481-500)
        from the device counters, with the reference's keys, value types and
        formulas, so a drop-in caller can format or add them.

        * 'killed': paths ended by RR (kernels.py:1145-1157), counted exactly
          (the reference's atomics are commented out, kernels.py:1193-1202,
          so its own 'killed' is always 0).
        * 'survived', 'avg_depth_killed', 'avg_depth_survived': 0 / 0.0, as in
          the reference: the device does not count paths that passed the RR
          test, nor depth sums. Their names are listed under 'uncounted'.
        * 'total_rr_paths' = killed + survived, as in the reference
          (renderer.py:488). 'kill_rate' is killed / paths x 100, the share of
          all traced paths that Russian roulette ended (0.0 when none were
          traced): the reference's killed / total_rr_paths would read 100 %
          whenever anything was killed, because survived is uncounted here, so
          that formula is not published.
        * Extra keys: 'paths', 'depth_cap' (paths ended by the depth / wave
          budget), 'uncounted'."""
        c = self.integrator.read_counters() or {}
        killed, survived = int(c.get('rr', 0)), 0
        total = killed + survived
        paths = int(c.get('paths', 0))
        return {'killed': killed, 'survived': survived, 'total_rr_paths': total,
                'kill_rate': 100.0 * killed / paths if paths else 0.0,
                'avg_depth_killed': 0.0, 'avg_depth_survived': 0.0,
                'paths': paths, 'depth_cap': int(c.get('depth_cap', 0)),
                'uncounted': ('survived', 'avg_depth_killed', 'avg_depth_survived')}

    def _get_average_depth(self):
        """Mean ray segments per path (renderer.py:473-479 reports the mean
        depth-loop count; a segment is one traversal of that loop)."""
        c = self.integrator.read_counters() or {}
        return c['segments'] / c['paths'] if c.get('paths') else 0.0

    def _print_depth_stats(self):
        """Depth statistics block of renderer.py:502-523."""
        c = self.integrator.read_counters() or {}
        n = c.get('paths', 0)
        if not n:
            return
        print('\nDepth Statistics:')
        print(f'  Average path segments: {c["segments"] / n:.2f} (max depth: {self.max_depth})')
        print(f'  Russian Roulette terminations: {c["rr"]:,} ({100.0 * c["rr"] / n:.1f}%)')
        print(f'  Max depth terminations: {c["depth_cap"]:,} ({100.0 * c["depth_cap"] / n:.1f}%)')
        print(f'  Total paths traced: {n:,}')

    def print_statistics(self):
        if not self.sample_times:
            return
        tot = sum(self.sample_times)
        avg = tot / len(self.sample_times)
        pps = self.cam.img_width * self.cam.img_height / avg if avg > 0 else 0.0
        c = self.integrator.read_counters() or {}
        print('\nPERFORMANCE SUMMARY')
        print(f'Total Render Time: {tot:6.2f}s')
        print(f'Throughput: {pps / 1e6:8.2f} Msamples/s')
        if c.get('paths'):
            print(f'Segments/sample: {c["segments"] / c["paths"]:.3f} | '
                  f'medium traversals/sample: {c["medium"] / c["paths"]:.3f}')
        self._print_depth_stats()
        if self._is_adaptive() and self.adaptive_passes and self._adaptive is not None:
            px = self.cam.img_width * self.cam.img_height
            uniform = px * self._adaptive['max_spp']
            print('\nAdaptive passes (active tiles | samples traced | share of a uniform '
                  f'{self._adaptive["max_spp"]}-spp render):')
            total = 0
            for q in self.adaptive_passes:
                total += q['traced']
                print(f'  pass {q["pass"] + 1:3d}: {q["active_tiles"]:7d} | {q["traced"]:13,} | '
                      f'{100.0 * q["traced"] / uniform:6.2f}%')
            print(f'  total: {total:,} of {uniform:,} samples ({100.0 * total / uniform:.1f}%)')
        if self.denoise_seconds is not None:
            print(f'Denoise Time: {1e3 * self.denoise_seconds:8.2f}ms')
        if self.guide_trace_seconds is not None:
            print(f'Guide Trace Time: {1e3 * self.guide_trace_seconds:8.2f}ms')

    _print_stats = print_statistics

    # -------------------------------------------------- live preview (GUI, out of scope)
    def setup_live_preview(self, update_interval_ms=500):
        """renderer.py:593-616 opens a Tk window here. The Tk GUI is out of
        scope, so this records the interval and opens nothing;
        callers such as InteractiveViewer keep working headless."""
        self.update_interval_ms = update_interval_ms
        self.preview_window = None
        self.last_preview_update = 0.0

    def update_preview_if_needed(self):
        """renderer.py:618-648: no window was opened (setup_live_preview), so
        there is nothing to refresh; use image_u8() for the current image."""
        return None


TaichiRenderer = MI355XRenderer  # drop-in name (render_server.taichi_renderer.TaichiRenderer)
