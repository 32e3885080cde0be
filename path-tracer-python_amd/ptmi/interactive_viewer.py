"""Headless InteractiveViewer (reference: src/render_server/interactive_viewer.py:18-451).

The reference's vol2_final_scene / cornell_box / cornell_smoke entry points
(scenes.py:1068, 1144, 1242) drive the renderer through
``InteractiveViewer(world, cam, path).render_interactive()``: progressive
accumulation up to ``cam.samples_per_pixel``, orbit-camera rotation that
restarts accumulation, and the image written at the end divided by
``cam.samples_per_pixel`` (renderer.py:436-442). This class keeps that API and
those effects on the MI355X integrator. The Tk preview window is out of scope
(SURVEY.md §2), so ``render_interactive`` returns once the sample budget is
reached instead of idling in a window; the mouse handlers stay callable with
any object carrying ``.x`` / ``.y`` so a host GUI can still drive them.

Progressive sampling launches ``display_interval`` samples per call (the
reference launches one per call, :389): sample i of a pixel is keyed by
(seed, pixel, i), so the accumulated image is bit-identical however the
samples are batched.

``InteractiveViewer(..., temporal=True, max_history=32)`` (no counterpart in
the reference): a camera move reprojects the accumulated history to the new
camera instead of clearing it. The default, temporal=False, is
the behaviour above, bit for bit.

``InteractiveViewer(..., temporal=True, motion=True)``: a scene update
(``update_primitives``) keeps the history too, carried to where every surface
point went. The default, motion=False, drops it as before.

``InteractiveViewer(..., temporal=True, validate=True, validate_spp=4)``: after a
reprojecting restart the first ``validate_spp`` samples are rendered apart and
judge the carried history, which is dropped where the light has changed
(``MI355XRenderer.render_validated``). The default,
validate=False, leaves the accumulator bit for bit what it was.
"""
from __future__ import annotations

import math
import statistics
import time

import torch

from .renderer import MI355XRenderer, _History


def spherical_from(lookfrom, lookat):
    """(radius, theta, phi) of lookfrom around lookat (interactive_viewer.py:52-71)."""
    off = lookfrom - lookat
    r = math.sqrt(off.x ** 2 + off.y ** 2 + off.z ** 2)
    theta = math.atan2(off.x, -off.z)
    phi = math.asin(off.y / r) if r > 0 else 0.0
    return r, theta, phi


def spherical_offset(radius, theta, phi):
    """Cartesian offset (x, y, z) of spherical coordinates (interactive_viewer.py:73-99)."""
    cp, sp = math.cos(phi), math.sin(phi)
    ct, st = math.cos(theta), math.sin(theta)
    return radius * cp * st, radius * sp, -radius * cp * ct


def orbit_step(theta, phi, delta_x, delta_y, velocity=(0.3, 0.3)):
    """New (theta, phi) after a mouse delta, phi clamped to +-89 deg (interactive_viewer.py:101-123)."""
    theta += math.radians(delta_x * velocity[0])
    phi += math.radians(delta_y * velocity[1])
    lim = math.radians(89.0)
    return theta, max(-lim, min(lim, phi))


class InteractiveViewer(MI355XRenderer):
    def __init__(self, world, cam, img_path: str, temporal: bool = False, max_history: float = 32,
                 motion: bool = False, validate: bool = False, validate_spp: int = 4, **kwargs):
        if motion and not temporal:
            raise ValueError('motion=True keeps the temporal history across scene updates: it needs temporal=True')
        if validate and not temporal:
            raise ValueError('validate=True validates the temporal history after a restart: it needs temporal=True')
        if int(validate_spp) < 2:
            raise ValueError('validate_spp must be at least 2: one fresh sample has no variance to judge by')
        super().__init__(world, cam, img_path, **kwargs)
        # temporal=True: a camera move reprojects the accumulated history to the
        # new camera instead of clearing it (MI355XRenderer.reproject_history,
        # DESIGN.md §15). The samples then always go through the stats path.
        self.temporal = bool(temporal)
        self.max_history = float(max_history)
        self.history_fraction = None  # pixels with history after the last reprojection
        self._sample_origin = 0  # RNG sample index of current_sample == 0: rises across restarts
        # what the last render was seen with (renderer._History): its camera and
        # guides. motion=True: update_primitives carries the history across the
        # update, so also its id image, and, once the scene has
        # been updated since that render, the primitive rows it was rendered with.
        self._history = None
        self.motion = bool(motion)
        self._history_kept = False  # the last restart reprojected: the next render keeps accum / stats
        # validate=True: the first validate_spp samples after a reprojecting restart go through
        # render_validated, which says how much of the history they kept
        self.validate = bool(validate)
        self.validate_spp = int(validate_spp)
        self.mouse_down = False
        self.last_mouse_x = 0
        self.last_mouse_y = 0
        self.last_camera_update_time = 0
        self.camera_update_interval = 0.05
        self.rotation_velocity = (0.3, 0.3)
        self._camera_radius = 0.0
        self._camera_theta = 0.0
        self._camera_phi = 0.0
        self._initialize_spherical_coords()
        self.is_rendering_active = True
        self.preview_window = None

    # ----------------------------------------------------------- orbit camera
    def _initialize_spherical_coords(self):
        self._camera_radius, self._camera_theta, self._camera_phi = spherical_from(self.cam.lookfrom,
                                                                                   self.cam.lookat)

    def _spherical_to_cartesian(self, radius, theta, phi):
        x, y, z = spherical_offset(radius, theta, phi)
        return type(self.cam.lookfrom - self.cam.lookat)(x, y, z)

    def rotate_camera(self, delta_x, delta_y):
        self._camera_theta, self._camera_phi = orbit_step(self._camera_theta, self._camera_phi, delta_x, delta_y,
                                                          self.rotation_velocity)
        offset = self._spherical_to_cartesian(self._camera_radius, self._camera_theta, self._camera_phi)
        self.cam.lookfrom = self.cam.lookat + offset
        self.cam.initialize()
        self._upload_camera_to_gpu()

    @property
    def next_sample_index(self):
        """RNG sample index of the next sample rendered: current_sample, plus,
        in a temporal viewer, the samples rendered before the restarts."""
        return self._sample_origin + self.current_sample

    def _restart_with_history(self, what='Camera rotated'):
        """The temporal restart: the rendered history reprojected to the
        camera uploaded (and, in a motion viewer, the scene updated) since.
        _history stays that of the last camera samples were rendered at, so a further restart with no
        sample in between (the next step of one drag) reprojects that same
        rendered history again (reproject_history(again=True)) instead of
        resampling the reprojected one. current_sample restarts at 0 as the
        progress count; the sample index goes on from _sample_origin, so no
        pixel draws the streams of its history again."""
        again = self._history_kept and self.current_sample == 0
        self._sample_origin += self.current_sample
        self.current_sample = 0
        self.sample_times = []
        self.render_start_time = time.time()
        # (a history with rows, of a scene updated since it was rendered, takes the motion-aware form)
        self.history_fraction = self._reproject_from(self._history, again, max_history=self.max_history)
        self._history_kept = True
        self.integrator.reset_counters()
        self.is_rendering_active = True
        print(f"\n{'─' * 60}\n{what} - history reprojected to {100.0 * self.history_fraction:.1f}% of the "
              f"pixels (at most {self.max_history:g} samples each)\n{'─' * 60}")

    def restart_rendering(self):
        if self.temporal and self.stats is not None and self._history is not None and \
                (self.current_sample > 0 or self._history_kept):
            return self._restart_with_history()
        self._history_kept = False
        self.render_start_time = time.time()
        self._restart_image()  # after a render with target_error, error estimates and tile states start over too
        self.is_rendering_active = True
        print(f"\n{'─' * 60}\nCamera rotated - restarting render from sample 0\n{'─' * 60}")

    def update_primitives(self, spheres=None, quads=None, triangles=None, rebuild=False, rebuild_growth=None,
                          builder='host'):
        """MI355XRenderer.update_primitives, ``rebuild``, ``rebuild_growth`` and
        ``builder`` included. What becomes of the temporal
        history is ``_change_scene``'s rule."""
        threshold = self._rebuild_threshold(rebuild, rebuild_growth, builder)

        def change():
            self._apply_update(spheres, quads, triangles)
            return self._rebuild_scene(builder) if self._wants_rebuild(rebuild, threshold) else None
        return self._change_scene(change, 'Scene updated')

    def update_materials(self, spheres=None, quads=None, triangles=None, media=None):
        """MI355XRenderer.update_materials. What becomes of the
        temporal history is ``_change_scene``'s rule."""
        def change():
            self._apply_materials(spheres, quads, triangles, media)
        return self._change_scene(change, 'Materials updated')

    def rebuild_bvh(self, builder='host'):
        """MI355XRenderer.rebuild_bvh, the temporal history treated as by ``update_primitives``."""
        self._rebuild_threshold(False, None, builder)
        return self._change_scene(lambda: self._rebuild_scene(builder), 'BVH rebuilt')

    def _change_scene(self, change, what):
        """Run ``change()``, which alters the scene and returns a rebuild's row
        maps or None. Without ``motion`` the temporal history is dropped with
        the image. A ``motion=True`` viewer that has a rendered
        history keeps it: the history is reprojected from the camera, guides,
        ids and primitive rows it was rendered with to the current camera and
        scene, its ids and rows carried to the new device order
        first if the BVH was rebuilt, by the rule of ``_restart_with_history``:
        a second change, or a camera move, with no sample in between
        reprojects the rendered history again, not the reprojected one."""
        if self.motion and self.stats is not None and self._history is not None and \
                self._history.ids is not None and (self.current_sample > 0 or self._history_kept):
            if self._history.rows is None:  # the scene still is what the history was rendered with
                self._history.rows = self.dscene.primitive_rows()
            maps = change()
            if maps is not None:
                self._history = self._history_across_rebuild(self._history, maps)
            return self._restart_with_history(what)
        self._after_scene_change(None, change(), {})
        self._history, self._history_kept = None, False
        self.history_fraction = None
        self.render_start_time = time.time()
        self.is_rendering_active = True

    # ------------------------------------------------------- mouse handlers
    def on_mouse_down(self, event):
        self.mouse_down = True
        self.last_mouse_x, self.last_mouse_y = event.x, event.y

    def on_mouse_up(self, event):
        self.mouse_down = False

    def on_mouse_drag(self, event):
        if not self.mouse_down:
            return
        now = time.time()
        if now - self.last_camera_update_time < self.camera_update_interval:
            self.last_mouse_x, self.last_mouse_y = event.x, event.y
            return
        self.last_camera_update_time = now
        dx, dy = event.x - self.last_mouse_x, event.y - self.last_mouse_y
        self.last_mouse_x, self.last_mouse_y = event.x, event.y
        if dx == 0 and dy == 0:
            return
        self.rotate_camera(dx, dy)
        self.restart_rendering()

    def setup_interactive_preview(self, update_interval_ms=16):
        """No window here (Tk preview is out of scope); kept for API compatibility."""
        self.update_interval_ms = update_interval_ms

    def update_preview_if_needed(self):
        return None

    # ------------------------------------------------------------ rendering
    def render_interactive(self, target_error=None, min_spp=16):
        """Progressive render to cam.samples_per_pixel, then write the image
        (interactive_viewer.py:327-451, headless). With ``target_error`` the
        samples accumulate through the stats path (per-pixel error estimates,
        MI355XRenderer.render_adaptive) and the render stops early once every
        tile has min_spp samples and an error of at most target_error; the
        image then divides by the samples rendered. target_error=None is the
        reference's behaviour.

        In a ``temporal=True`` viewer the samples go through the stats path
        with or without ``target_error``, the guides of the camera are traced
        once, and a call that follows a reprojecting restart keeps the
        history: sample index ``next_sample_index`` goes on where the last
        render stopped, and the image divides each pixel by its own count.

        With the renderer's ``shutter`` (a keyword of the constructor, like
        ``slice_spp``) every step goes through the same pose sequence as the
        renderer's own calls (MI355XRenderer._trace)."""
        spp = int(self.cam.samples_per_pixel)
        print('\nInteractiveViewer')
        print(f'Resolution: {self.cam.img_width}x{self.cam.img_height} | Max Samples: {spp} | Depth: {self.max_depth}')
        print(f'Spheres: {self.num_spheres} | BVH Nodes: {self.num_bvh_nodes}')
        self._upload_camera_to_gpu()
        t0 = time.time()
        stats_path = target_error is not None or self.temporal
        validate_now = self.validate and self.temporal and self._history_kept
        if self.temporal and self._history_kept:
            # after a reprojecting restart: accum / stats hold the history, so the
            # warm-up sample goes to a scratch accumulator and nothing is cleared
            self.integrator.render_mk(self.frame, torch.empty_like(self.accum), 0, 1)
            torch.cuda.synchronize(self.dscene.device)
            self._integrator_label = 'adaptive-megakernel'
        else:
            self.render_sample(0)  # warm-up sample, cleared (interactive_viewer.py:355-359)
            torch.cuda.synchronize(self.dscene.device)
            self.clear_accumulation_buffer()
            if stats_path:
                self._integrator_label = 'adaptive-megakernel'
                self._adaptive = None  # no pass schedule: not resumable as a render_adaptive() run
                self._adaptive_reset()
        if self.temporal:  # the guides of this camera, traced once: what a later restart reprojects by
            self._history = _History(self.frame.cam, *(self.guides_ids() if self.motion else (self.guides(),)))
            self._history_kept = False
        self.integrator.reset_counters()
        print(f'  Kernel Warmup: {(time.time() - t0) * 1000:6.2f}ms')
        self.setup_interactive_preview()
        display_interval = max(1, spp // 20)
        total_pixels = self.cam.img_width * self.cam.img_height
        print(f"\nRendering Progress:\n{'─' * 60}")
        self.render_start_time = time.time()
        if validate_now and self.is_rendering_active and min(self.validate_spp, spp - self.current_sample) >= 2:
            n = min(self.validate_spp, spp - self.current_sample)
            kept = self.render_validated(n)
            torch.cuda.synchronize(self.dscene.device)
            print(f'{self.current_sample:4d}/{spp} validated the history: reprojected to '
                  f'{100.0 * self.history_fraction:.1f}% of the pixels, {100.0 * kept:.1f}% of its samples kept')
        while self.is_rendering_active and self.current_sample < spp:
            n = min(display_interval - self.current_sample % display_interval, spp - self.current_sample)
            if self.current_sample == 0:
                n = 1  # the reference prints sample 1
            t = time.time()
            if not stats_path:
                self._trace(self.integrator.render_mk, self.accum, begin=self.current_sample, count=n)
            else:
                self._trace(self.integrator.render_mk_stats, self.accum, self.stats, begin=self.next_sample_index,
                            count=n)
                if target_error is not None:
                    left = self.integrator.tile_update(self.frame, self.stats, target_error, min_spp, spp,
                                                       self._tiles)
            torch.cuda.synchronize(self.dscene.device)
            dt = (time.time() - t) / n
            self.sample_times += [dt] * n
            self.current_sample += n
            elapsed = time.time() - self.render_start_time
            avg = sum(self.sample_times) / len(self.sample_times)
            thr = total_pixels / avg if avg > 0 else 0.0
            print(f'{self.current_sample:4d}/{spp} ({self.current_sample / spp * 100:5.1f}%) │ {dt * 1000:5.1f}ms │ '
                  f'Elapsed: {elapsed:5.1f}s │ Throughput: {thr / 1e6:5.2f}M pix/s │ '
                  f'ETA: {(spp - self.current_sample) * avg:4.1f}s')
            if target_error is not None and left == 0 and self.current_sample < spp:
                print(f"{'─' * 60}\n✓ Every tile within the target error {target_error:g} "
                      f'after {self.current_sample} samples')
                self.is_rendering_active = False
                break
        if self.current_sample >= spp:
            print(f"{'─' * 60}\n✓ Reached max samples ({spp})")
            self.is_rendering_active = False
        self._print_render_summary()
        self._sync_gpu_to_cpu()
        self.write_image()

    def _sync_gpu_to_cpu(self):
        """renderer.py:566-573: nothing to copy (the accumulator stays on the GPU)."""
        return None

    def _print_render_summary(self):
        if not self.sample_times:
            return
        st = self.sample_times
        avg = statistics.mean(st)
        total_pixels = self.cam.img_width * self.cam.img_height
        c = self.integrator.read_counters() or {}
        print(f"\n{'═' * 60}\nRENDER SUMMARY\n{'═' * 60}")
        print(f'Resolution:       {self.cam.img_width} x {self.cam.img_height} ({total_pixels:,} pixels)')
        print(f'Samples:          {self.current_sample} / {self.cam.samples_per_pixel}')
        print(f'Max Ray Depth:    {self.max_depth}')
        if c.get('paths'):
            print(f'Avg Path Depth:   {c["segments"] / c["paths"]:.2f}')
        print(f'Scene Complexity: {self.num_spheres} spheres, {self.num_bvh_nodes} BVH nodes')
        print(f'Total Render Time:  {time.time() - self.render_start_time:6.2f}s')
        print(f'Sample Time: mean {avg * 1000:6.2f}ms | median {statistics.median(st) * 1000:6.2f}ms | '
              f'min {min(st) * 1000:6.2f}ms | max {max(st) * 1000:6.2f}ms')
        print(f'Pixels/sec:       {total_pixels / avg / 1e6 if avg > 0 else 0.0:6.2f} Mpix/s')
