"""MI355X-native render path for the reference's per-pixel integrator loop.

`HipRenderer` is the Python face of the C-ABI (include/pbr_hip.h): upload a reference-shaped scene
(`scenes.Scene`), then `render()` runs Whitted/Path/VolPath on the GPU — the counterpart of
`Integrator::Render(const Scene&, double&)` (Integrator/Integrator.h:14).  The C++ host mirror of
the reference classes lives in include/pbr/ (see INTEGRATION.md).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, scenes  # noqa: F401

__all__ = ["AdaptiveRender", "HipRenderer", "ProgressiveRender", "TemporalRender", "capi", "scenes", "tile_grid", "tiles_for_rank"]


class PbrError(RuntimeError):
    pass


class HipRenderer:
    def __init__(self, device: int = 0):
        self.lib = capi.load_library()
        self.ctx = C.c_void_p()
        rc = self.lib.pbr_hip_create(device, C.byref(self.ctx))
        if rc != capi.PBR_OK:
            raise PbrError(f"pbr_hip_create failed ({rc}); a GPU is required — there is no CPU fallback")

    def _check(self, rc, what):
        if rc != capi.PBR_OK:
            raise PbrError(f"{what} failed ({rc}): {self.lib.pbr_hip_last_error(self.ctx).decode()}")

    def sync(self):
        """Wait for asynchronous frames; raises if one stopped at a safety bound (pbr_hip_sync)."""
        self._check(self.lib.pbr_hip_sync(self.ctx), "sync")

    def close(self):
        if self.ctx:
            self.lib.pbr_hip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, scene: "scenes.Scene"):
        self._desc = scene.desc()
        self._desc.abi_version = self.lib.pbr_hip_abi_version()   # (an older A/B build: same descriptors)
        self._scene = scene
        self._check(self.lib.pbr_hip_upload_scene(self.ctx, C.byref(self._desc)), "upload_scene")

    @staticmethod
    def n_pixels(rdesc) -> int:
        if rdesc.n_tiles:
            return sum((rdesc.tiles[i].x1 - rdesc.tiles[i].x0) * (rdesc.tiles[i].y1 - rdesc.tiles[i].y0)
                       for i in range(rdesc.n_tiles))
        return rdesc.camera.width * rdesc.camera.height

    def render(self, rdesc, rgb=True, rgba=True, stats=False):
        """Returns (rgb float32 [n,3], rgba uint8 [n,4], RenderStats) in packed tile order."""
        n = self.n_pixels(rdesc)
        out_rgb = np.empty((n, 3), dtype=np.float32) if rgb else None
        out_rgba = np.empty((n, 4), dtype=np.uint8) if rgba else None
        st = capi.RenderStats()
        rdesc.outputs_on_device = 0
        rdesc.collect_stats = int(stats)
        self._check(self.lib.pbr_hip_render(self.ctx, C.byref(rdesc),
                                             out_rgb.ctypes.data if rgb else None,
                                             out_rgba.ctypes.data if rgba else None, C.byref(st)), "render")
        return out_rgb, out_rgba, st

    def render_device(self, rdesc, rgb_ptr: int, rgba_ptr: int, stream: int | None = None, stats=False,
                      sync=True):
        """Render straight into device buffers (e.g. torch tensors' data_ptr()) on `stream`.

        sync=False (and stats=False): the frame is only enqueued on `stream` — the caller
        synchronises — and None is returned; frames then run back to back on the device."""
        rdesc.outputs_on_device = 1
        rdesc.stream = stream
        rdesc.collect_stats = int(stats)
        st = capi.RenderStats() if (sync or stats) else None
        self._check(self.lib.pbr_hip_render(self.ctx, C.byref(rdesc), rgb_ptr or None, rgba_ptr or None,
                                            C.byref(st) if st is not None else None), "render")
        return st

    def render_frames(self, rdesc, rgb_ptrs, rgba_ptrs, stream: int | None = None):
        """n frames of one descriptor into device buffers (pbr_hip_render_frames): their chunks
        continue one rotation over the lanes with no join between frames.  Asynchronous; `stream`
        reaches its tail when every frame is done; wait_frame orders another stream after one."""
        rgb_ptrs, rgba_ptrs = self._out_lists("render_frames", rgb_ptrs, rgba_ptrs)
        n = max(len(rgb_ptrs), len(rgba_ptrs))
        if n == 0:
            raise ValueError("render_frames: no output buffers")
        self._check(self.lib.pbr_hip_render_frames(self.ctx, C.byref(self._device_desc(rdesc, stream)), n,
                                                   self._ptr_array(rgb_ptrs), self._ptr_array(rgba_ptrs)), "render_frames")

    @staticmethod
    def _out_lists(who, rgb_ptrs, rgba_ptrs):
        rgb_ptrs, rgba_ptrs = list(rgb_ptrs or []), list(rgba_ptrs or [])
        if rgb_ptrs and rgba_ptrs and len(rgb_ptrs) != len(rgba_ptrs):
            raise ValueError(f"{who}: {len(rgb_ptrs)} float outputs but {len(rgba_ptrs)} RGBA8 outputs")
        return rgb_ptrs, rgba_ptrs

    @staticmethod
    def _ptr_array(ptrs):
        return (C.c_void_p * len(ptrs))(*[p or None for p in ptrs]) if ptrs else None

    @staticmethod
    def _device_desc(rdesc, stream):
        """What the asynchronous entry points run: device outputs on `stream`, no stats.  The caller's
        descriptor is left as it was: the settings go on a copy (its tile pointer still refers to the
        caller's arrays, which rdesc keeps alive for the call)."""
        d = type(rdesc).from_buffer_copy(rdesc)
        d.outputs_on_device = 1
        d.stream = stream
        d.collect_stats = 0
        return d

    @staticmethod
    def sample_budget(rdesc) -> int:
        """The sampler's samplesPerPixel for rdesc.spp: Sobol rounds it up to a power of two."""
        spp = int(rdesc.spp)
        if rdesc.sampler == capi.SAMPLER_SOBOL and spp > 0:
            spp = 1 << (spp - 1).bit_length()
        return spp

    @staticmethod
    def _pass_budget(who, rdesc) -> int:
        if rdesc.sampler == capi.SAMPLER_TABLE:
            raise ValueError(f"{who}: no passes over a sample table")
        return HipRenderer.sample_budget(rdesc)

    @staticmethod
    def _check_pass(who, rdesc, first_sample, samples, n_passes, accum_ptr, accum_floats, samples_arg="samples"):
        """A window of n_passes passes of `samples` samples from first_sample, refused before any library
        call unless it lies in the sampler's budget; returns the three as ints, and the budget."""
        first_sample, samples, n_passes = int(first_sample), int(samples), int(n_passes)
        if samples < 1:
            raise ValueError(f"{who}: {samples_arg} must be >= 1")
        if first_sample < 0:
            raise ValueError(f"{who}: first_sample must be >= 0")
        if not accum_ptr:
            raise ValueError(f"{who}: accum is required (a device buffer of {accum_floats} float32 per pixel)")
        budget = HipRenderer._pass_budget(who, rdesc)
        end = first_sample + n_passes * samples
        if end > budget:
            raise ValueError(f"{who}: samples [{first_sample}, {end}) run past the budget of {budget} samples per pixel")
        return first_sample, samples, n_passes, budget

    def render_passes(self, rdesc, first_sample, samples_per_pass, accum_ptr, rgb_ptrs=None, rgba_ptrs=None,
                      n_passes=None, stream: int | None = None):
        """Sample passes over a carried accumulator (pbr_hip_render_passes): n_passes passes of
        samples_per_pass samples per pixel from sample number first_sample, added in sample order onto
        accum (device, 6 float32 per pixel: Σ Li.rgb, Σ Li.rgb²).  Pass p's image — the sum over all
        samples so far divided by their count — goes to rgb_ptrs[p] / rgba_ptrs[p] (device pointers;
        a list, or an entry, may be None).  rdesc.spp stays the whole budget.  n_passes defaults to the
        length of the output lists.  Asynchronous, as render_frames; wait_frame(stream, p) orders
        another stream after pass p."""
        rgb_ptrs, rgba_ptrs = self._out_lists("render_passes", rgb_ptrs, rgba_ptrs)
        n = max(len(rgb_ptrs), len(rgba_ptrs)) if n_passes is None else int(n_passes)
        if n < 1:
            raise ValueError("render_passes: no passes (give n_passes or output buffers)")
        for name, ptrs in (("rgb_ptrs", rgb_ptrs), ("rgba_ptrs", rgba_ptrs)):
            if ptrs and len(ptrs) != n:
                raise ValueError(f"render_passes: {len(ptrs)} {name} for {n} passes")
        first_sample, samples_per_pass, n, _ = self._check_pass("render_passes", rdesc, first_sample, samples_per_pass, n,
                                                                accum_ptr, 6, samples_arg="samples_per_pass")
        d = self._device_desc(rdesc, stream)
        self._check(self.lib.pbr_hip_render_passes(self.ctx, C.byref(d), first_sample, samples_per_pass, n, accum_ptr,
                                                   self._ptr_array(rgb_ptrs), self._ptr_array(rgba_ptrs)), "render_passes")

    @staticmethod
    def _check_mirror_bounces(who, mirror_bounces) -> int:
        b = int(mirror_bounces)
        if b < 0 or b > capi.AOV_MAX_MIRROR_BOUNCES:
            raise ValueError(f"{who}: mirror_bounces must be in 0..{capi.AOV_MAX_MIRROR_BOUNCES}")
        return b

    def render_aov(self, rdesc, first_sample, samples, accum_ptr, out_ptr=None, stream: int | None = None, mirror_bounces=0):
        """A feature pass (pbr_hip_render_aov): for samples [first_sample, first_sample + samples) of every
        pixel, the albedo (3), hit (1), shading normal (3) and distance (1) of the first surface the camera
        sample sees, added in sample order onto accum (device, capi.AOV_CHANNELS float32 per pixel, packed
        tile order; not read when first_sample == 0).  out_ptr (device, 8 float32 per pixel, or None)
        receives the image over all samples so far: mean albedo, coverage, mean normal (not renormalised),
        mean distance of the samples that hit.  rdesc.spp stays the whole budget; the descriptor's
        integrator, depth and light strategy are not read.  Asynchronous, ordered as render_passes;
        wait_frame(stream, 0) orders another stream after it.
        mirror_bounces = B > 0 (pbr_hip_render_aov_mirrors): up to B mirror bounces are followed, and the
        surface at the end of the chain is recorded, with the product of the albedos along the chain, its own
        normal (not reflected back) and the summed distance; 0 is the plain pass."""
        b = self._check_mirror_bounces("render_aov", mirror_bounces)
        first_sample, samples, _, _ = self._check_pass("render_aov", rdesc, first_sample, samples, 1, accum_ptr, 8)
        d = self._device_desc(rdesc, stream)
        if b == 0:   # (the plain entry point: the same call underneath, and an older A/B build has it)
            rc = self.lib.pbr_hip_render_aov(self.ctx, C.byref(d), first_sample, samples, accum_ptr, out_ptr or None)
        else:
            rc = self.lib.pbr_hip_render_aov_mirrors(self.ctx, C.byref(d), b, first_sample, samples, accum_ptr, out_ptr or None)
        self._check(rc, "render_aov")

    def mirror_step_host(self, hits, kr):
        """One mirror step of the followed feature pass per hit, on the CPU (pbr_hip_mirror_step_host: the
        kernel's own function compiled for the host; no GPU call): hits an array of capi.SurfaceHit as query()
        returns them, kr [n, 3] the mirror's Kr at each.  Returns (rays [n, 7] float32: o, d, tMax of the
        continuation, zeros where the step is refused; followed [n] int32)."""
        return capi.mirror_step_host(hits, kr, self.lib)

    @staticmethod
    def _check_denoise(who, width, height, samples, have_counts, iterations, sigma_l, sigma_n, sigma_z, min_samples=2):
        """The frame and filter parameters of a denoise call, refused before any library call; returns
        them as a capi.Denoise (demodulate left 0).  min_samples: 1 with the spatial variance estimate."""
        width, height, samples, iterations = int(width), int(height), int(samples), int(iterations)
        if width < 1 or height < 1:
            raise ValueError(f"{who}: width and height must be >= 1")
        if width * height >= 1 << 31:
            raise ValueError(f"{who}: width * height must be below 2^31")
        if not 1 <= iterations <= 8:
            raise ValueError(f"{who}: iterations must be 1..8")
        for name, v in (("sigma_l", sigma_l), ("sigma_n", sigma_n), ("sigma_z", sigma_z)):
            if not float(v) > 0.0:   # (a NaN fails the comparison)
                raise ValueError(f"{who}: {name} must be > 0 (inf switches the term off)")
        if not have_counts and samples < 2 and min_samples >= 2:
            raise ValueError(f"{who}: samples must be >= 2 (a variance needs two), or give per-pixel counts")
        if not have_counts and samples < 1:
            raise ValueError(f"{who}: samples must be >= 1, or give per-pixel counts")
        return capi.Denoise(width, height, iterations, 0, float(sigma_l), float(sigma_n), float(sigma_z))

    @staticmethod
    def _check_spatial(who, spatial):
        """spatial=(min_count, radius) of a denoise call, refused before any library call; returns it as a
        capi.SpatialVariance."""
        try:
            min_count, radius = spatial
            min_count, radius = int(min_count), int(radius)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: spatial must be (min_count, radius) or None") from None
        if not 2 <= min_count <= 64:
            raise ValueError(f"{who}: spatial min_count must be 2..64")
        if not 1 <= radius <= 3:
            raise ValueError(f"{who}: spatial radius must be 1..3")
        return capi.SpatialVariance(min_count, radius)

    def denoise(self, width, height, samples, accum_ptr, aov_ptr, rgb_ptr=None, rgba_ptr=None, var_ptr=None, counts_ptr=None,
                iterations=5, demodulate=True, sigma_l=4.0, sigma_n=0.4, sigma_z=1.0, stream: int | None = None,
                spatial=None):
        """The edge-avoiding à-trous filter (pbr_hip_denoise) over a width x height frame in raster order:
        accum_ptr the 6 sums per pixel of render_passes, aov_ptr the 8-float image of render_aov, counts_ptr
        (or None: every pixel took `samples`) the int32 per-pixel sample counts of render_adaptive.
        `iterations` levels of a 5x5 B3-spline wavelet, level i stepping 2^i pixels, edge-stopped on
        luminance against the local variance (sigma_l), the mean normal (sigma_n) and the distance against
        its slope (sigma_z); demodulate filters colour / albedo.  Outputs (device pointers, at least one):
        rgb_ptr 3 float32 per pixel, rgba_ptr its 8-bit film transform, var_ptr the filtered variance.
        spatial=(min_count, radius), suggested (4, 1): the spatial variance estimate (pbr_hip_denoise_sv) before
        level 0 — a pixel with 1 <= count < min_count takes its variance from the (2 radius + 1)^2 pixels
        around it, so frames of one sample per pixel are filtered; samples may then be 1.
        Asynchronous, ordered as render_aov; wait_frame(stream, 0) orders another stream after it."""
        sv = None if spatial is None else self._check_spatial("denoise", spatial)
        p = self._check_denoise("denoise", width, height, samples, bool(counts_ptr), iterations, sigma_l, sigma_n, sigma_z,
                                min_samples=2 if sv is None else 1)
        if not accum_ptr or not aov_ptr:
            raise ValueError("denoise: accum (6 float32 per pixel) and aov (8 float32 per pixel) are required")
        if not (rgb_ptr or rgba_ptr or var_ptr):
            raise ValueError("denoise: no output buffer")
        p.demodulate = 1 if demodulate else 0
        if sv is None:
            self._check(self.lib.pbr_hip_denoise(self.ctx, C.byref(p), int(samples), counts_ptr or None, accum_ptr, aov_ptr,
                                                 rgb_ptr or None, rgba_ptr or None, var_ptr or None, stream), "denoise")
        else:
            self._check(self.lib.pbr_hip_denoise_sv(self.ctx, C.byref(p), C.byref(sv), int(samples), counts_ptr or None,
                                                    accum_ptr, aov_ptr, rgb_ptr or None, rgba_ptr or None, var_ptr or None,
                                                    stream), "denoise")

    def spatial_variance_host(self, width, height, samples, accum, aov, counts=None, spatial=(4, 1), demodulate=True,
                              sigma_n=0.4, sigma_z=1.0):
        """The variance plane level 0 of denoise(spatial=...) reads, on the CPU over numpy arrays
        (pbr_hip_spatial_variance_host: the device's prepare and estimate functions compiled for the host; no GPU
        call): [n] float32.  spatial=None gives prepare's own variance."""
        sv = None if spatial is None else self._check_spatial("spatial_variance_host", spatial)
        p = self._check_denoise("spatial_variance_host", width, height, samples, counts is not None, 1, 1.0, sigma_n, sigma_z,
                                min_samples=2 if sv is None else 1)
        n = p.width * p.height
        arrays = []
        for name, a, dt, ch in (("accum", accum, np.float32, 6), ("aov", aov, np.float32, 8), ("counts", counts, np.int32, 1)):
            if a is None:
                if name != "counts":
                    raise ValueError(f"spatial_variance_host: {name} is required")
                arrays.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=dt)
            if a.size != n * ch:
                raise ValueError(f"spatial_variance_host: {name} holds {a.size} values, expected {n} x {ch}")
            arrays.append(a)
        acc, img, cnt = arrays
        p.demodulate = 1 if demodulate else 0
        out = np.empty(n, np.float32)
        rc = self.lib.pbr_hip_spatial_variance_host(C.byref(p), None if sv is None else C.byref(sv), int(samples),
                                                    cnt.ctypes.data if cnt is not None else None, acc.ctypes.data,
                                                    img.ctypes.data, out.ctypes.data)
        if rc != capi.PBR_OK:
            raise PbrError(f"spatial_variance_host failed ({rc})")
        return out

    @staticmethod
    def _check_temporal(who, width, height, samples, have_counts, max_history, tol_z, tol_n, cur, prev):
        """The frame, parameters and cameras of a temporal merge, refused before any library call; returns
        them as a capi.Temporal (demodulate left 0).  cur and prev: capi.camera_matrices() of the two cameras."""
        width, height, samples, max_history = int(width), int(height), int(samples), int(max_history)
        if width < 1 or height < 1:
            raise ValueError(f"{who}: width and height must be >= 1")
        if width * height >= 1 << 31:
            raise ValueError(f"{who}: width * height must be below 2^31")
        if not 1 <= max_history <= 1 << 20:
            raise ValueError(f"{who}: max_history must be 1..2^20")
        for name, v in (("tol_z", tol_z), ("tol_n", tol_n)):
            if not float(v) >= 0.0:   # (a NaN fails the comparison)
                raise ValueError(f"{who}: {name} must be >= 0")
        if not have_counts and samples < 1:
            raise ValueError(f"{who}: samples must be >= 1, or give per-pixel counts")
        p = capi.Temporal(width, height, max_history, 0, float(tol_z), float(tol_n))
        for name, cam in (("cur", cur), ("prev", prev)):
            if cam is None or len(cam) != 3:
                raise ValueError(f"{who}: {name} must be (raster_to_world, world_to_raster, eye) of capi.camera_matrices")
        for field, name, a, n in (("cur_raster_to_world", "cur's raster_to_world", cur[0], 16), ("cur_eye", "cur's eye", cur[2], 3),
                                  ("prev_world_to_raster", "prev's world_to_raster", prev[1], 16), ("prev_eye", "prev's eye", prev[2], 3)):
            a = np.asarray(a, dtype=np.float32).reshape(-1)
            if a.size != n:
                raise ValueError(f"{who}: {name} must hold {n} floats")
            if np.isnan(a).any():
                raise ValueError(f"{who}: a NaN in {name}")
            getattr(p, field)[:] = a.tolist()
        return p

    def temporal(self, width, height, samples, accum_cur_ptr, aov_cur_ptr, counts_prev_ptr, accum_prev_ptr, aov_prev_ptr,
                 accum_out_ptr, counts_out_ptr, cur, prev, counts_cur_ptr=None, motion_ptr=None, rgb_ptr=None, rgba_ptr=None,
                 max_history=32, demodulate=True, tol_z=0.05, tol_n=0.1, stream: int | None = None):
        """Temporal accumulation (pbr_hip_temporal) over a width x height frame in raster order: the previous
        frame's sums (accum_prev 6 float32 per pixel, counts_prev int32 per pixel, aov_prev its 8-float feature
        image) are reprojected into this frame's (accum_cur, aov_cur; counts_cur or None: every pixel took
        `samples`) and merged as at most max_history samples of history; accum_out / counts_out (which may be
        the current buffers, never the previous ones) have the format of accum and counts, so
        denoise(counts_ptr=counts_out) works on them.  cur and prev are capi.camera_matrices() of this frame's
        and the previous frame's camera.  Optional outputs: motion_ptr 2 float32 per pixel, rgb_ptr 3 float32,
        rgba_ptr its 8-bit film transform.  All device pointers.  Asynchronous, ordered as denoise;
        wait_frame(stream, 0) orders another stream after it."""
        p = self._check_temporal("temporal", width, height, samples, bool(counts_cur_ptr), max_history, tol_z, tol_n, cur, prev)
        if not (accum_cur_ptr and aov_cur_ptr and counts_prev_ptr and accum_prev_ptr and aov_prev_ptr):
            raise ValueError("temporal: accum_cur, aov_cur, counts_prev, accum_prev and aov_prev are required")
        if not (accum_out_ptr and counts_out_ptr):
            raise ValueError("temporal: accum_out and counts_out are required")
        for out in (accum_out_ptr, counts_out_ptr, motion_ptr, rgb_ptr, rgba_ptr):
            if out and out in (counts_prev_ptr, accum_prev_ptr, aov_prev_ptr):
                raise ValueError("temporal: an output buffer is one of the previous frame's")
        p.demodulate = 1 if demodulate else 0
        self._check(self.lib.pbr_hip_temporal(self.ctx, C.byref(p), int(samples), counts_cur_ptr or None, accum_cur_ptr,
                                              aov_cur_ptr, counts_prev_ptr, accum_prev_ptr, aov_prev_ptr, accum_out_ptr,
                                              counts_out_ptr, motion_ptr or None, rgb_ptr or None, rgba_ptr or None, stream),
                    "temporal")

    def temporal_host(self, width, height, samples, accum_cur, aov_cur, counts_prev, accum_prev, aov_prev, cur, prev,
                      counts_cur=None, max_history=32, demodulate=True, tol_z=0.05, tol_n=0.1):
        """The same merge on the CPU over numpy arrays (pbr_hip_temporal_host: the device's per-pixel function
        compiled for the host; no GPU call): returns (accum_out [n, 6] float32, counts_out [n] int32,
        motion [n, 2] float32).  The inputs are left as they are."""
        p = self._check_temporal("temporal_host", width, height, samples, counts_cur is not None, max_history, tol_z, tol_n,
                                 cur, prev)
        n = p.width * p.height
        arrays = []
        for name, a, dt, ch in (("accum_cur", accum_cur, np.float32, 6), ("aov_cur", aov_cur, np.float32, 8),
                                ("counts_prev", counts_prev, np.int32, 1), ("accum_prev", accum_prev, np.float32, 6),
                                ("aov_prev", aov_prev, np.float32, 8), ("counts_cur", counts_cur, np.int32, 1)):
            if a is None:
                if name != "counts_cur":
                    raise ValueError(f"temporal_host: {name} is required")
                arrays.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=dt)
            if a.size != n * ch:
                raise ValueError(f"temporal_host: {name} holds {a.size} values, expected {n} x {ch}")
            arrays.append(a)
        a_cur, f_cur, c_prev, a_prev, f_prev, c_cur = arrays
        p.demodulate = 1 if demodulate else 0
        out, cnt, mot = np.empty((n, 6), np.float32), np.empty(n, np.int32), np.empty((n, 2), np.float32)
        rc = self.lib.pbr_hip_temporal_host(C.byref(p), int(samples), c_cur.ctypes.data if c_cur is not None else None,
                                            a_cur.ctypes.data, f_cur.ctypes.data, c_prev.ctypes.data, a_prev.ctypes.data,
                                            f_prev.ctypes.data, out.ctypes.data, cnt.ctypes.data, mot.ctypes.data)
        if rc != capi.PBR_OK:
            raise PbrError(f"temporal_host failed ({rc})")
        return out, cnt, mot

    @staticmethod
    def _check_rule(who, tolerance, floor):
        tolerance, floor = float(tolerance), float(floor)
        if not tolerance >= 0.0:   # (a NaN fails the comparison)
            raise ValueError(f"{who}: tolerance must be >= 0, not {tolerance}")
        if not floor >= 0.0:
            raise ValueError(f"{who}: floor must be >= 0, not {floor}")
        return tolerance, floor

    def adaptive_select(self, n_pixels, samples_done, tolerance, floor, accum_ptr, list_out_ptr, list_in_ptr=None, n_in=0,
                        err_out_ptr=None) -> int:
        """The stopping rule of adaptive sampling over an accumulator (pbr_hip_adaptive_select): of the
        n_in pixels in list_in (device int32, ascending; None: all n_pixels) those still active at
        samples_done samples go, in order, to list_out (device int32); returns their number.  err_out
        (device float32 per frame pixel) receives the error estimate E of the pixels considered.
        Synchronous."""
        n_pixels, samples_done, n_in = int(n_pixels), int(samples_done), int(n_in)
        if samples_done < 2:
            raise ValueError("adaptive_select: samples_done must be >= 2")
        if n_pixels < 1 or n_pixels >= 1 << 31:
            raise ValueError("adaptive_select: n_pixels must be in [1, 2^31)")
        tolerance, floor = self._check_rule("adaptive_select", tolerance, floor)
        if not accum_ptr or not list_out_ptr:
            raise ValueError("adaptive_select: accum and list_out are required (device buffers)")
        if list_in_ptr and not 0 <= n_in <= n_pixels:
            raise ValueError(f"adaptive_select: n_in {n_in} outside [0, {n_pixels}]")
        n = C.c_int(0)
        self._check(self.lib.pbr_hip_adaptive_select(self.ctx, n_pixels, samples_done, tolerance, floor, accum_ptr,
                                                     list_in_ptr or None, n_in, list_out_ptr, C.byref(n), err_out_ptr or None),
                    "adaptive_select")
        return n.value

    def render_passes_list(self, rdesc, first_sample, samples, list_ptr, n_list, accum_ptr, rgb_ptr=None, rgba_ptr=None,
                           stream: int | None = None):
        """One pass of `samples` samples from sample number first_sample for the n_list pixels in list
        (device int32, ascending packed pixel indices) only (pbr_hip_render_passes_list).  accum, rgb
        and rgba are whole-frame device buffers; entries of unlisted pixels are not written.  Waits for
        the list's run count, then queues the pass as render_passes does."""
        first_sample, samples, _, _ = self._check_pass("render_passes_list", rdesc, first_sample, samples, 1, accum_ptr, 6)
        n_list = int(n_list)
        if n_list < 0 or n_list > self.n_pixels(rdesc):
            raise ValueError(f"render_passes_list: n_list {n_list} outside [0, {self.n_pixels(rdesc)}]")
        if n_list and not list_ptr:
            raise ValueError("render_passes_list: list is required (a device buffer of int32 pixel indices)")
        d = self._device_desc(rdesc, stream)
        self._check(self.lib.pbr_hip_render_passes_list(self.ctx, C.byref(d), first_sample, samples, list_ptr or None, n_list,
                                                        accum_ptr, rgb_ptr or None, rgba_ptr or None), "render_passes_list")

    @staticmethod
    def _check_adaptive(who, rdesc, min_samples, samples_per_round, tolerance, floor):
        budget = HipRenderer._pass_budget(who, rdesc)
        if rdesc.spp < 1:
            raise ValueError(f"{who}: rdesc.spp (the sample budget) must be >= 1")
        min_samples, samples_per_round = int(min_samples), int(samples_per_round)
        if min_samples < 2 or min_samples > budget:
            raise ValueError(f"{who}: min_samples {min_samples} outside [2, {budget}] (the budget)")
        if samples_per_round < 1:
            raise ValueError(f"{who}: samples_per_round must be >= 1")
        tolerance, floor = HipRenderer._check_rule(who, tolerance, floor)
        return capi.Adaptive(min_samples, samples_per_round, tolerance, floor)

    def render_adaptive(self, rdesc, min_samples, samples_per_round, tolerance, floor, accum_ptr, counts_ptr, rgb_ptr=None,
                        rgba_ptr=None, stream: int | None = None):
        """A whole adaptive render (pbr_hip_render_adaptive): every pixel takes min_samples samples,
        then rounds of samples_per_round for the pixels the stopping rule leaves active, up to the
        budget rdesc.spp.  accum (6 float32 per pixel), counts (int32 per pixel), rgb, rgba: device
        buffers.  Synchronous; returns the capi.AdaptiveResult."""
        a = self._check_adaptive("render_adaptive", rdesc, min_samples, samples_per_round, tolerance, floor)
        if not accum_ptr or not counts_ptr:
            raise ValueError("render_adaptive: accum and counts are required (device buffers)")
        d = self._device_desc(rdesc, stream)
        res = capi.AdaptiveResult()
        self._check(self.lib.pbr_hip_render_adaptive(self.ctx, C.byref(d), C.byref(a), accum_ptr, counts_ptr, rgb_ptr or None,
                                                     rgba_ptr or None, C.byref(res)), "render_adaptive")
        return res

    def wait_frame(self, stream: int | None, f: int):
        """Make `stream` wait for frame f of the last render_frames call, or pass f of the last
        render_passes call (pbr_hip_wait_frame)."""
        self._check(self.lib.pbr_hip_wait_frame(self.ctx, stream, f), "wait_frame")

    def set_schedule(self, kernels=capi.KERNELS_AUTO, chunk_log2=0, lanes=0, fuse_camera=capi.FUSE_AUTO, serial=False):
        """How later frames are cut into launches (pbr_hip_set_schedule); no arguments = the measured
        default; serial=True runs every launch on the caller's stream in turn (measurement).  Results
        are the same bits under every schedule."""
        s = capi.Schedule(kernels, chunk_log2, lanes, fuse_camera, int(serial))
        self._check(self.lib.pbr_hip_set_schedule(self.ctx, C.byref(s)), "set_schedule")

    def last_chunks(self) -> dict:
        """The chunk plan the last render, render_frames or render_passes call ran (pbr_hip_last_chunks):
        lanes, chunk_pixels, n_chunks, queue capacities, the budget computed for that call, the bytes
        the lane buffers hold, whether lane 0 ran on the context's stream and whether the camera was
        fused.  lanes == 0 and n_chunks == 0: the call ran the megakernel."""
        out = capi.ChunkPlan()
        self._check(self.lib.pbr_hip_last_chunks(self.ctx, C.byref(out)), "last_chunks")
        return out.as_dict()

    @staticmethod
    def plan_chunks(integrator, n_pixels, spp, max_depth, **kw) -> dict:
        """The plan for such a frame without rendering it (capi.plan_chunks; no GPU call)."""
        return capi.plan_chunks(integrator, n_pixels, spp, max_depth, **kw)

    def set_profiling(self, on: bool = True):
        """Start (on) or stop a per-kernel measurement window (pbr_hip_set_profiling)."""
        self._check(self.lib.pbr_hip_set_profiling(self.ctx, int(on)), "set_profiling")

    def get_profile(self) -> dict:
        """Per kernel family of the window: launches, summed HIP-event ms, work units, algorithmic
        HBM bytes and raw counters (pbr_hip_get_profile); starts a new window."""
        arr = (capi.KernelProfile * 32)()
        n = C.c_int()
        self._check(self.lib.pbr_hip_get_profile(self.ctx, arr, 32, C.byref(n)), "get_profile")
        return {arr[i].name.decode(): {"launches": arr[i].launches, "ms": arr[i].ms, "units": int(arr[i].units),
                                       "bytes": int(arr[i].bytes), "counts": [int(c) for c in arr[i].counts]}
                for i in range(min(n.value, 32))}

    def get_bvh(self):
        nn, npr = C.c_int(), C.c_int()
        self._check(self.lib.pbr_hip_get_bvh(self.ctx, None, C.byref(nn), None, C.byref(npr)), "get_bvh")
        nodes = np.empty(nn.value * 32, dtype=np.uint8)
        ids = np.empty(npr.value, dtype=np.int32)
        self._check(self.lib.pbr_hip_get_bvh(self.ctx, nodes.ctypes.data, C.byref(nn), capi.iptr(ids), C.byref(npr)),
                    "get_bvh")
        return nodes, ids

    def set_bvh_build(self, where: int):
        """Which SAH builder the next upload runs: capi.BVH_BUILD_DEVICE (default) or BVH_BUILD_HOST."""
        self._check(self.lib.pbr_hip_set_bvh_build(self.ctx, where), "set_bvh_build")

    def bvh_build_info(self) -> dict:
        """The last upload's BVH build: builder, wall ms, device kernel ms (pbr_hip_bvh_build_info)."""
        w, ms, kms = C.c_int(), C.c_double(), C.c_double()
        self._check(self.lib.pbr_hip_bvh_build_info(self.ctx, C.byref(w), C.byref(ms), C.byref(kms)), "bvh_build_info")
        return {"where": "device" if w.value == capi.BVH_BUILD_DEVICE else "host", "ms": ms.value,
                "kernel_ms": kms.value}

    def build_bvh(self, prim_bounds, where=capi.BVH_BUILD_DEVICE, max_prims=1):
        """BVHAccel's SAH build over [n, 6] primitive world bounds (pbr_hip_build_bvh): returns
        (LinearBVHNode bytes [n_nodes*32], ordered prim ids, {"ms", "kernel_ms"})."""
        b = np.ascontiguousarray(prim_bounds, dtype=np.float32).reshape(-1, 6)
        n = b.shape[0]
        nodes = np.zeros(max(1, 2 * n - 1) * 32, dtype=np.uint8)
        ids = np.zeros(max(1, n), dtype=np.int32)
        nn = C.c_int()
        ms = (C.c_double * 2)()
        self._check(self.lib.pbr_hip_build_bvh(self.ctx, where, n, capi.fptr(b), max_prims, nodes.ctypes.data,
                                                C.byref(nn), capi.iptr(ids), ms), "build_bvh")
        return nodes[:nn.value * 32], ids[:n], {"ms": ms[0], "kernel_ms": ms[1]}

    def sampler_values(self, width, height, spp, queries, sampler=capi.SAMPLER_HALTON):
        q = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1, 4)
        out = np.empty(q.shape[0], dtype=np.float32)
        self._check(self.lib.pbr_hip_sampler_values(self.ctx, sampler, width, height, spp, q.shape[0], capi.iptr(q),
                                                    capi.fptr(out)), "sampler_values")
        return out

    def sample_index(self, width, height, spp, px_py_sample, sampler=capi.SAMPLER_HALTON):
        """GlobalSampler::GetIndexForSample on the device: int64 [n]."""
        q = np.ascontiguousarray(px_py_sample, dtype=np.int32).reshape(-1, 3)
        out = np.empty(q.shape[0], dtype=np.int64)
        self._check(self.lib.pbr_hip_sample_index(self.ctx, sampler, width, height, spp, q.shape[0], capi.iptr(q),
                                                  out.ctypes.data_as(C.POINTER(C.c_int64))), "sample_index")
        return out

    def sample_dimensions(self, width, height, index, px_py_dim, sampler=capi.SAMPLER_HALTON):
        """GlobalSampler::SampleDimension(index, dim) on the device (pixel for Sobol's dims 0, 1): float32 [n]."""
        idx = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
        q = np.ascontiguousarray(px_py_dim, dtype=np.int32).reshape(-1, 3)
        assert idx.shape[0] == q.shape[0]
        out = np.empty(q.shape[0], dtype=np.float32)
        self._check(self.lib.pbr_hip_sample_dimensions(self.ctx, sampler, width, height, q.shape[0],
                                                       idx.ctypes.data_as(C.POINTER(C.c_int64)), capi.iptr(q),
                                                       capi.fptr(out)), "sample_dimensions")
        return out

    def camera_rays(self, cam, pfilm):
        pf = np.ascontiguousarray(pfilm, dtype=np.float32).reshape(-1, 2)
        out = np.empty((pf.shape[0], 6), dtype=np.float32)
        self._check(self.lib.pbr_hip_camera_rays(self.ctx, C.byref(cam), pf.shape[0], capi.fptr(pf), capi.fptr(out)),
                    "camera_rays")
        return out

    def query(self, rays, any_hit=False, prim=-1):
        """Scene::Intersect / IntersectP (prim >= 0: GeometricPrimitive::Intersect of that primitive)
        with the SurfaceInteraction fields of each hit: an array of capi.SurfaceHit."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
        out = (capi.SurfaceHit * max(1, r.shape[0]))()
        self._check(self.lib.pbr_hip_query(self.ctx, r.shape[0], capi.fptr(r), int(any_hit), int(prim), out), "query")
        return out[:r.shape[0]]

    def bounds(self, prim=-1):
        """Scene::WorldBound (prim = -1) or GeometricPrimitive::WorldBound: (lo[3], hi[3])."""
        b = np.empty(6, dtype=np.float32)
        self._check(self.lib.pbr_hip_bounds(self.ctx, int(prim), capi.fptr(b)), "bounds")
        return b[:3], b[3:]

    def li(self, rdesc, rays, px_py_sample_dim, depth=0):
        """SamplerIntegrator::Li on the device for caller-given rays: float32 [n, 3]."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
        q = np.ascontiguousarray(px_py_sample_dim, dtype=np.int32).reshape(-1, 4)
        assert q.shape[0] == r.shape[0]
        out = np.empty((r.shape[0], 3), dtype=np.float32)
        self._check(self.lib.pbr_hip_li(self.ctx, C.byref(rdesc), r.shape[0], capi.fptr(r), capi.iptr(q), int(depth),
                                        capi.fptr(out)), "li")
        return out

    def intersect(self, rays, any_hit=False):
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
        out = np.empty((r.shape[0], 5), dtype=np.float32)
        self._check(self.lib.pbr_hip_intersect(self.ctx, r.shape[0], capi.fptr(r), capi.fptr(out), int(any_hit)),
                    "intersect")
        return out

    def intersect_walk(self, rays, walk, any_hit=False, seg_counts=None, seg_cap=None):
        """intersect() through one production BVH walk (capi.WALK_*): the same [n, 5] records.
        seg_counts (capi.WALK_SEGMENTS ints) and seg_cap lay the rays out as the segmented queue of
        the queue walks."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
        out = np.empty((r.shape[0], 5), dtype=np.float32)
        sc = None
        if seg_counts is not None:
            sc = np.ascontiguousarray(seg_counts, dtype=np.int32)
            if sc.shape != (capi.WALK_SEGMENTS,):
                raise ValueError(f"seg_counts: {capi.WALK_SEGMENTS} counts")
        self._check(self.lib.pbr_hip_intersect_walk(self.ctx, int(walk), r.shape[0], capi.fptr(r), capi.fptr(out), int(any_hit),
                                                    int(seg_cap or 0), capi.iptr(sc) if sc is not None else None),
                    "intersect_walk")
        return out

    def bsdf(self, queries, variant=capi.BSDF_VARIANT_ALL):
        """BSDF::f, Pdf and Sample_f of the uploaded scene's materials on caller-given directions,
        under the lobe mask and template source of one production shading kernel
        (capi.BSDF_VARIANT_*): capi.bsdf_query_dtype records in, capi.bsdf_record_dtype records out."""
        q = np.ascontiguousarray(queries, dtype=capi.bsdf_query_dtype()).reshape(-1)
        out = np.zeros(q.shape[0], dtype=capi.bsdf_record_dtype())
        self._check(self.lib.pbr_hip_bsdf(self.ctx, int(variant), q.shape[0], q.ctypes.data, out.ctypes.data), "bsdf")
        return out

    def phase_hg(self, queries):
        """HenyeyGreenstein::p and Sample_p on the device: [n, 9] (g, wo, wi, u0, u1) → [n, 5]
        (p(wo, wi), the sampled wi, its value)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 9)
        out = np.zeros((q.shape[0], 5), dtype=np.float32)
        self._check(self.lib.pbr_hip_phase_hg(self.ctx, q.shape[0], capi.fptr(q), capi.fptr(out)), "phase_hg")
        return out


class ProgressiveRender:
    """A render that proceeds in sample passes and can stop, show, checkpoint and resume.

    Owns the accumulator of HipRenderer.render_passes as a torch tensor on the renderer's device
    ([n_pixels, 6] float32 in the descriptor's packed tile order: Σ Li.rgb, Σ Li.rgb²).  The image
    after k samples is the bits of a whole render whose sampler's first k samples are these; at
    rdesc.spp samples it is HipRenderer.render's.

    features=True: every step also advances a feature accumulator ([n_pixels, 8] float32, the sums of
    HipRenderer.render_aov) over the same samples; features() gives the denoiser inputs, and state() /
    restore() carry it under the key "features".  mirror_bounces=B: those feature passes follow up to B
    mirror bounces (render_aov's mirror_bounces).  The state does not record B: restoring a state taken under
    another mirror_bounces continues sums of a different rule, and is the caller's error (not detected)."""

    def __init__(self, renderer: HipRenderer, rdesc, device=None, features=False, mirror_bounces=0):
        self.mirror_bounces = HipRenderer._check_mirror_bounces("ProgressiveRender", mirror_bounces)
        self.budget = HipRenderer._pass_budget("ProgressiveRender", rdesc)
        if rdesc.spp < 1:
            raise ValueError("ProgressiveRender: rdesc.spp (the sample budget) must be >= 1")
        self.renderer = renderer
        self.rdesc = rdesc
        self.n_pixels = HipRenderer.n_pixels(rdesc)
        self.samples_done = 0
        self._device = device
        self._features = bool(features)
        self._accum = self._rgb = self._rgba = self._stream = self._aov = self._aov_img = None
        self._dn_rgb = self._dn_rgba = None

    def _check_step(self, n_samples, passes):
        n_samples, passes = int(n_samples), int(passes)
        if n_samples < 1 or passes < 1:
            raise ValueError("ProgressiveRender.step: n_samples and passes must be >= 1")
        if self.samples_done + n_samples * passes > self.budget:
            raise ValueError(f"ProgressiveRender.step: {self.samples_done} samples done, {n_samples * passes} more run "
                             f"past the budget of {self.budget}")
        return n_samples, passes

    def _buffers(self):
        import torch
        if self._accum is None:
            dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            self._accum = torch.zeros((self.n_pixels, 6), dtype=torch.float32, device=dev)
            self._rgb = torch.empty((self.n_pixels, 3), dtype=torch.float32, device=dev)
            self._rgba = torch.empty((self.n_pixels, 4), dtype=torch.uint8, device=dev)
            if self._features:
                self._aov = torch.zeros((self.n_pixels, capi.AOV_CHANNELS), dtype=torch.float32, device=dev)
                self._aov_img = torch.zeros((self.n_pixels, capi.AOV_CHANNELS), dtype=torch.float32, device=dev)
            # the passes run on a stream of their own (the library takes a real stream handle; torch's
            # default stream has none), ordered against the caller's current stream by events
            self._stream = torch.cuda.Stream(dev)
        return torch

    def step(self, n_samples, passes=1):
        """`passes` passes of n_samples samples per pixel in one call; returns the (rgb, rgba) device
        tensors of the image after the last one.  They are reused by the next step.  Asynchronous: the
        call returns once the passes are enqueued, and the current torch stream is made to wait for them,
        so work queued on it afterwards (a copy to the host, a display kernel) sees the finished image."""
        n_samples, passes = self._check_step(n_samples, passes)
        torch = self._buffers()
        current = torch.cuda.current_stream(self._accum.device)
        self._stream.wait_stream(current)   # (the accumulator's initialisation or restore, readers of the last image)
        rgb = [None] * (passes - 1) + [self._rgb.data_ptr()]
        rgba = [None] * (passes - 1) + [self._rgba.data_ptr()]
        self.renderer.render_passes(self.rdesc, self.samples_done, n_samples, self._accum.data_ptr(), rgb, rgba,
                                    stream=self._stream.cuda_stream)
        if self._features:   # (one feature pass over the step's samples, behind its passes on the same stream)
            self.renderer.render_aov(self.rdesc, self.samples_done, n_samples * passes, self._aov.data_ptr(),
                                     self._aov_img.data_ptr(), stream=self._stream.cuda_stream,
                                     mirror_bounces=self.mirror_bounces)
        current.wait_stream(self._stream)
        self.samples_done += n_samples * passes
        return self._rgb, self._rgba

    def features(self) -> dict:
        """The feature buffers over the samples done so far, as views of one device tensor (reused by the
        next step): albedo [n, 3], coverage [n], normal [n, 3] (the mean shading normal, not renormalised),
        depth [n] (the mean distance of the samples that hit; 0 where none did)."""
        if not self._features:
            raise ValueError("ProgressiveRender.features: constructed with features=False")
        if self.samples_done < 1:
            raise ValueError("ProgressiveRender.features needs at least one step")
        self._buffers()
        f = self._aov_img
        return {"albedo": f[:, 0:3], "coverage": f[:, 3], "normal": f[:, 4:7], "depth": f[:, 7]}

    def denoise(self, iterations=5, demodulate=True, sigma_l=4.0, sigma_n=0.4, sigma_z=1.0, spatial=None):
        """The image after the samples done so far, filtered (HipRenderer.denoise over the carried sums
        and the feature image): (rgb [n, 3] float32, rgba [n, 4] uint8) device tensors of its own, reused
        by the next call.  Needs features=True, at least 2 samples per pixel (1 with spatial=(min_count,
        radius), the spatial variance estimate), and a descriptor without tiles (the filter works on a whole
        frame in raster order).  Asynchronous as step()."""
        if not self._features:
            raise ValueError("ProgressiveRender.denoise: constructed with features=False")
        if self.rdesc.n_tiles:
            raise ValueError("ProgressiveRender.denoise: a tiled descriptor (the filter would stop at the tiles' borders)")
        if spatial is not None:
            HipRenderer._check_spatial("ProgressiveRender.denoise", spatial)
            if self.samples_done < 1:
                raise ValueError("ProgressiveRender.denoise needs at least 1 sample per pixel")
        elif self.samples_done < 2:
            raise ValueError("ProgressiveRender.denoise needs at least 2 samples per pixel")
        w, h = self.rdesc.camera.width, self.rdesc.camera.height
        HipRenderer._check_denoise("ProgressiveRender.denoise", w, h, self.samples_done, False, iterations, sigma_l, sigma_n,
                                   sigma_z, min_samples=2 if spatial is None else 1)
        torch = self._buffers()
        if self._dn_rgb is None:
            self._dn_rgb = torch.empty((self.n_pixels, 3), dtype=torch.float32, device=self._accum.device)
            self._dn_rgba = torch.empty((self.n_pixels, 4), dtype=torch.uint8, device=self._accum.device)
        current = torch.cuda.current_stream(self._accum.device)
        self._stream.wait_stream(current)   # (readers of the last denoised image)
        self.renderer.denoise(w, h, self.samples_done, self._accum.data_ptr(), self._aov_img.data_ptr(),
                              rgb_ptr=self._dn_rgb.data_ptr(), rgba_ptr=self._dn_rgba.data_ptr(), iterations=iterations,
                              demodulate=demodulate, sigma_l=sigma_l, sigma_n=sigma_n, sigma_z=sigma_z,
                              stream=self._stream.cuda_stream, spatial=spatial)
        current.wait_stream(self._stream)
        return self._dn_rgb, self._dn_rgba

    def variance(self):
        """Per-pixel, per-channel sample variance [n_pixels, 3] (device tensor) from the two carried
        sums: (Σ L² − (Σ L)²/k) / (k − 1).  An estimate: float32 sums of squares lose low bits the
        exact variance would keep, so tiny negative values are clamped to zero."""
        if self.samples_done < 2:
            raise ValueError("ProgressiveRender.variance needs at least 2 samples per pixel")
        torch = self._buffers()
        k = float(self.samples_done)
        s, s2 = self._accum[:, :3], self._accum[:, 3:]
        return torch.clamp((s2 - s * s / k) / (k - 1.0), min=0.0)

    def state(self) -> dict:
        """A checkpoint: the accumulator as a numpy array and the samples done (waits for the device)."""
        self._buffers()
        st = {"samples_done": self.samples_done, "accum": self._accum.cpu().numpy().copy()}
        if self._features:
            st["features"] = self._aov.cpu().numpy().copy()
        return st

    def restore(self, state: dict):
        """Resume from state(): the same descriptor on any renderer holding the same scene."""
        acc = np.asarray(state["accum"], dtype=np.float32)
        done = int(state["samples_done"])
        if acc.shape != (self.n_pixels, 6):
            raise ValueError(f"ProgressiveRender.restore: accumulator of shape {acc.shape}, expected {(self.n_pixels, 6)}")
        if done < 0 or done > self.budget:
            raise ValueError(f"ProgressiveRender.restore: {done} samples done outside the budget of {self.budget}")
        feat = None
        if self._features:
            if "features" not in state:
                raise ValueError("ProgressiveRender.restore: the state carries no feature accumulator")
            feat = np.asarray(state["features"], dtype=np.float32)
            if feat.shape != (self.n_pixels, capi.AOV_CHANNELS):
                raise ValueError(f"ProgressiveRender.restore: feature accumulator of shape {feat.shape}, expected "
                                 f"{(self.n_pixels, capi.AOV_CHANNELS)}")
        torch = self._buffers()
        self._accum.copy_(torch.from_numpy(np.ascontiguousarray(acc)))
        if feat is not None:
            self._aov.copy_(torch.from_numpy(np.ascontiguousarray(feat)))
        self.samples_done = done


class AdaptiveRender:
    """A render that stops each pixel once its estimated error is small enough (adaptive sampling).

    Every pixel takes min_samples samples; then, round after round, the pixels whose error estimate —
    the variance of the pixel mean summed over the channels — still exceeds (tolerance × max(mean summed
    over the channels, floor))² take samples_per_round more, up to the budget rdesc.spp.  A pixel that
    passes the test once has stopped for good.  Owns the accumulator ([n_pixels, 6] float32: Σ Li.rgb,
    Σ Li.rgb²) and the per-pixel sample counts ([n_pixels] int32) as torch tensors on the renderer's
    device, in the descriptor's packed tile order; a pixel's image is the bits of a whole render at the
    pixel's count.  A checkpoint is those two tensors (state / restore)."""

    def __init__(self, renderer: HipRenderer, rdesc, min_samples=4, samples_per_round=4, tolerance=0.02, floor=1e-3,
                 device=None):
        self.params = HipRenderer._check_adaptive("AdaptiveRender", rdesc, min_samples, samples_per_round, tolerance, floor)
        self.renderer = renderer
        self.rdesc = rdesc
        self.budget = HipRenderer.sample_budget(rdesc)
        self.n_pixels = HipRenderer.n_pixels(rdesc)
        self.samples_done = 0      # the largest count any pixel has reached
        self.rounds = 0            # passes rendered, the full-frame first one included
        self.active = None         # pixels the last select found active (None: no select yet)
        self._device = device
        self._accum = self._counts = self._rgb = self._rgba = self._stream = None

    def _buffers(self):
        import torch
        if self._accum is None:
            dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            self._accum = torch.zeros((self.n_pixels, 6), dtype=torch.float32, device=dev)
            self._counts = torch.zeros((self.n_pixels,), dtype=torch.int32, device=dev)
            self._rgb = torch.zeros((self.n_pixels, 3), dtype=torch.float32, device=dev)
            self._rgba = torch.zeros((self.n_pixels, 4), dtype=torch.uint8, device=dev)
            self._stream = torch.cuda.Stream(dev)   # (the library takes a real stream handle: ProgressiveRender)
        return torch

    def run(self, max_rounds=None):
        """Runs to the end — nothing active, or the budget reached — and returns the (rgb, rgba) device
        tensors.  A fresh render with max_rounds None is one pbr_hip_render_adaptive call.  With
        max_rounds, at most that many passes are rendered (the full-frame first one counts) and run() may
        be called again; this, and a run after restore(), drive the same rounds from here through
        adaptive_select and render_passes_list, and leave the same bits.  Synchronous."""
        if max_rounds is not None and int(max_rounds) < 1:
            raise ValueError("AdaptiveRender.run: max_rounds must be >= 1")
        torch = self._buffers()
        torch.cuda.synchronize(self._accum.device)   # (the tensors' initialisation or restore)
        r, p, st = self.renderer, self.params, self._stream.cuda_stream
        if self.samples_done == 0 and max_rounds is None:
            res = r.render_adaptive(self.rdesc, p.min_samples, p.samples_per_round, p.tolerance, p.floor,
                                    self._accum.data_ptr(), self._counts.data_ptr(), self._rgb.data_ptr(),
                                    self._rgba.data_ptr(), stream=st)
            self.samples_done, self.rounds, self.active = res.max_samples_done, res.rounds, int(res.active_at_end)
            return self._rgb, self._rgba
        left = None if max_rounds is None else int(max_rounds)
        if self.samples_done == 0:
            r.render_passes(self.rdesc, 0, p.min_samples, self._accum.data_ptr(), [self._rgb.data_ptr()],
                            [self._rgba.data_ptr()], stream=st)
            r.sync()
            self._counts.fill_(p.min_samples)
            self.samples_done, self.rounds = p.min_samples, 1
            left = None if left is None else left - 1
        # the pixels still in the running are those at the largest count; each round selects over them
        k = self.samples_done
        cur = torch.nonzero(self._counts == k).flatten().to(torch.int32)
        while left is None or left > 0:
            nxt = torch.empty_like(cur)
            torch.cuda.synchronize(self._accum.device)
            n = r.adaptive_select(self.n_pixels, k, p.tolerance, p.floor, self._accum.data_ptr(), nxt.data_ptr(),
                                  cur.data_ptr(), cur.numel()) if cur.numel() else 0
            self.active = n
            if n == 0 or k >= self.budget:
                break
            step = min(p.samples_per_round, self.budget - k)
            cur = nxt[:n]
            r.render_passes_list(self.rdesc, k, step, cur.data_ptr(), n, self._accum.data_ptr(), self._rgb.data_ptr(),
                                 self._rgba.data_ptr(), stream=st)
            r.sync()
            k += step
            self._counts[cur.long()] = k
            self.samples_done, self.rounds = k, self.rounds + 1
            left = None if left is None else left - 1
        torch.cuda.synchronize(self._accum.device)
        return self._rgb, self._rgba

    def sample_map(self):
        """The samples each pixel took so far: [n_pixels] int32 device tensor, packed tile order."""
        self._buffers()
        return self._counts

    def state(self) -> dict:
        """A checkpoint: the accumulator and the counts as numpy arrays (waits for the device)."""
        self._buffers()
        return {"accum": self._accum.cpu().numpy().copy(), "counts": self._counts.cpu().numpy().copy(), "rounds": self.rounds}

    def restore(self, state: dict):
        """Resume from state(): the same descriptor and parameters on any renderer holding the same
        scene.  The images are not part of a checkpoint: a restored pixel's is written again by the
        next pass that samples it."""
        acc = np.asarray(state["accum"], dtype=np.float32)
        cnt = np.asarray(state["counts"])
        if acc.shape != (self.n_pixels, 6):
            raise ValueError(f"AdaptiveRender.restore: accumulator of shape {acc.shape}, expected {(self.n_pixels, 6)}")
        if cnt.shape != (self.n_pixels,):
            raise ValueError(f"AdaptiveRender.restore: counts of shape {cnt.shape}, expected {(self.n_pixels,)}")
        if cnt.size and (cnt.min() < 0 or cnt.max() > self.budget):
            raise ValueError(f"AdaptiveRender.restore: counts outside the budget of {self.budget}")
        torch = self._buffers()
        self._accum.copy_(torch.from_numpy(np.ascontiguousarray(acc)))
        self._counts.copy_(torch.from_numpy(np.ascontiguousarray(cnt.astype(np.int32))))
        self.samples_done = int(cnt.max()) if cnt.size else 0
        self.rounds = int(state.get("rounds", 0))
        self.active = None


class TemporalRender:
    """A camera path at a few samples per frame, each frame carrying the frames before it (temporal
    accumulation, HipRenderer.temporal).

    frame(camera) renders samples_per_frame samples of every pixel under `camera` — frame f draws the
    sample numbers [s0, s0 + k), s0 = (f mod cycle) · k, so successive frames draw different samples —
    with their feature buffers, reprojects the history it holds (the merged sums, counts and feature image
    of the previous call, and that call's camera) into them, and keeps the result as the new history.
    Owns the sums ([n, 6] float32), counts ([n] int32) and feature images ([n, 8] float32) as torch tensors
    on the renderer's device, in raster order: the descriptor must have no tiles.  The scene is static;
    after a new upload call reset().  mirror_bounces=B: the feature pass of every frame follows up to B
    mirror bounces (render_aov's mirror_bounces), so that what a planar mirror shows is reprojected with the
    parallax of its mirror image instead of the mirror's own."""

    def __init__(self, renderer: HipRenderer, rdesc, samples_per_frame, cycle=16, max_history=32, demodulate=True,
                 tol_z=0.05, tol_n=0.1, device=None, mirror_bounces=0):
        self.mirror_bounces = HipRenderer._check_mirror_bounces("TemporalRender", mirror_bounces)
        k, cycle = int(samples_per_frame), int(cycle)
        if k < 1 or cycle < 1:
            raise ValueError("TemporalRender: samples_per_frame and cycle must be >= 1")
        budget = HipRenderer._pass_budget("TemporalRender", rdesc)
        if k * cycle > budget:
            raise ValueError(f"TemporalRender: {cycle} frames of {k} samples run past the budget of {budget} samples per "
                             f"pixel (rdesc.spp)")
        if rdesc.n_tiles:
            raise ValueError("TemporalRender: a tiled descriptor (the merge works on a whole frame in raster order)")
        w, h = rdesc.camera.width, rdesc.camera.height
        ident = (np.eye(4, dtype=np.float32),) * 2 + (np.zeros(3, np.float32),)
        HipRenderer._check_temporal("TemporalRender", w, h, k, False, max_history, tol_z, tol_n, ident, ident)
        self.renderer, self.rdesc = renderer, rdesc
        self.samples_per_frame, self.cycle = k, cycle
        self.params = dict(max_history=int(max_history), demodulate=bool(demodulate), tol_z=float(tol_z), tol_n=float(tol_n))
        self.width, self.height, self.n_pixels = w, h, w * h
        self.frames_done = 0
        self._device = device
        self._sets = self._aov_sum = self._motion = self._rgb = self._rgba = self._stream = None
        self._dn_rgb = self._dn_rgba = None
        self._hist = None          # index of the set that holds the history (None: no history)
        self._prev_cam = None      # capi.camera_matrices of the history's camera

    def _buffers(self):
        import torch
        if self._sets is None:
            dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            n = self.n_pixels
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            # two sets of (sums, counts, feature image): one holds the history, the other takes the frame
            self._sets = [(z((n, 6), torch.float32), z((n,), torch.int32), z((n, capi.AOV_CHANNELS), torch.float32))
                          for _ in range(2)]
            self._aov_sum = z((n, capi.AOV_CHANNELS), torch.float32)
            self._motion = z((n, 2), torch.float32)
            self._rgb = z((n, 3), torch.float32)
            self._rgba = z((n, 4), torch.uint8)
            self._stream = torch.cuda.Stream(dev)   # (the library takes a real stream handle: ProgressiveRender)
        return torch

    def reset(self):
        """Drops the history: the next frame is the plain samples_per_frame-sample frame."""
        self._hist = None
        self._prev_cam = None

    def frame(self, camera):
        """One frame under `camera` (a capi.CameraDesc of the descriptor's raster size): (rgb [n, 3] float32,
        rgba [n, 4] uint8) device tensors of the merged image, reused by the next frame.  Asynchronous as
        ProgressiveRender.step."""
        if camera.width != self.width or camera.height != self.height:
            raise ValueError(f"TemporalRender.frame: a {camera.width}x{camera.height} camera for a "
                             f"{self.width}x{self.height} frame")
        cam = capi.camera_matrices(camera, self.renderer.lib)
        torch = self._buffers()
        r, k, st = self.renderer, self.samples_per_frame, self._stream
        d = type(self.rdesc).from_buffer_copy(self.rdesc)
        d.camera = camera
        s0 = (self.frames_done % self.cycle) * k
        cur = 1 if self._hist == 0 else 0
        acc, cnt, img = self._sets[cur]
        hacc, hcnt, himg = self._sets[1 - cur]
        current = torch.cuda.current_stream(acc.device)
        st.wait_stream(current)   # (the tensors' initialisation, readers of the last image)
        with torch.cuda.stream(st):
            acc.zero_()
            self._aov_sum.zero_()
            if self._hist is None:
                hcnt.zero_()   # (no history: a count of 0 drops every tap)
        r.render_passes(d, s0, k, acc.data_ptr(), [None], [None], stream=st.cuda_stream)
        r.render_aov(d, s0, k, self._aov_sum.data_ptr(), None, stream=st.cuda_stream, mirror_bounces=self.mirror_bounces)
        with torch.cuda.stream(st):   # the feature image over these k samples (aov_out's formula)
            f = self._aov_sum
            img[:, 0:7] = f[:, 0:7] / torch.full_like(f[:, 0:7], float(k))   # (a tensor divisor: a true division)
            hit = f[:, 3]
            img[:, 7] = torch.where(hit > 0, f[:, 7] / hit, torch.zeros_like(hit))
        r.temporal(self.width, self.height, k, acc.data_ptr(), img.data_ptr(), hcnt.data_ptr(), hacc.data_ptr(), himg.data_ptr(),
                   acc.data_ptr(), cnt.data_ptr(), cam, self._prev_cam if self._prev_cam is not None else cam,
                   motion_ptr=self._motion.data_ptr(), rgb_ptr=self._rgb.data_ptr(), rgba_ptr=self._rgba.data_ptr(),
                   stream=st.cuda_stream, **self.params)
        current.wait_stream(st)
        self._hist, self._prev_cam = cur, cam
        self.frames_done += 1
        return self._rgb, self._rgba

    def history(self) -> dict:
        """The merged frame held as history, device tensors reused by later frames: sums [n, 6], counts [n],
        features [n, 8] (this frame's own feature image) and motion [n, 2] of the last merge."""
        if self._hist is None:
            raise ValueError("TemporalRender.history: no frame yet (or reset)")
        acc, cnt, img = self._sets[self._hist]
        return {"accum": acc, "counts": cnt, "features": img, "motion": self._motion}

    def denoise(self, iterations=5, demodulate=True, sigma_l=4.0, sigma_n=0.4, sigma_z=1.0, spatial=None):
        """The merged frame filtered (HipRenderer.denoise over the merged sums with counts = the merged
        counts): (rgb [n, 3] float32, rgba [n, 4] uint8) device tensors of its own.  spatial=(min_count,
        radius): the spatial variance estimate for the pixels whose history is shorter than min_count samples
        — the first frame, and every disoccluded pixel, at one sample per frame."""
        if self._hist is None:
            raise ValueError("TemporalRender.denoise: no frame yet (or reset)")
        if spatial is not None:
            HipRenderer._check_spatial("TemporalRender.denoise", spatial)
        HipRenderer._check_denoise("TemporalRender.denoise", self.width, self.height, 0, True, iterations, sigma_l, sigma_n,
                                   sigma_z)
        torch = self._buffers()
        acc, cnt, img = self._sets[self._hist]
        if self._dn_rgb is None:
            self._dn_rgb = torch.empty((self.n_pixels, 3), dtype=torch.float32, device=acc.device)
            self._dn_rgba = torch.empty((self.n_pixels, 4), dtype=torch.uint8, device=acc.device)
        current = torch.cuda.current_stream(acc.device)
        self._stream.wait_stream(current)   # (readers of the last denoised image)
        self.renderer.denoise(self.width, self.height, 0, acc.data_ptr(), img.data_ptr(), rgb_ptr=self._dn_rgb.data_ptr(),
                              rgba_ptr=self._dn_rgba.data_ptr(), counts_ptr=cnt.data_ptr(), iterations=iterations,
                              demodulate=demodulate, sigma_l=sigma_l, sigma_n=sigma_n, sigma_z=sigma_z,
                              stream=self._stream.cuda_stream, spatial=spatial)
        current.wait_stream(self._stream)
        return self._dn_rgb, self._dn_rgba


# Edge of the multi-GPU tiles.  Per-rank frame of an 8-GPU C2 job (slowest of 8 ranks, one GPU,
# tools/shard_sweep.sh): 64 → 3.14 ms, 32 → 3.07, 16 → 3.02; 32 keeps the tile list short.
TILE = 32


def tile_grid(width, height, tile=TILE):
    """TILE×TILE (32×32) pixel tiles in row-major order (SURVEY §8(e) suggests 64×64; 32×32 measured
    better, see the TILE comment)."""
    return [(x, y, min(x + tile, width), min(y + tile, height))
            for y in range(0, height, tile) for x in range(0, width, tile)]


def tiles_for_rank(width, height, rank, world, tile=TILE):
    """Round-robin tile ownership `tileId mod nGPU` so heavy regions spread over ranks."""
    return [t for i, t in enumerate(tile_grid(width, height, tile)) if i % world == rank]


def assemble(width, height, tiles, packed, channels):
    """Scatter a packed per-tile buffer back into a row-major frame."""
    frame = np.zeros((height, width, channels), dtype=packed.dtype)
    pos = 0
    for (x0, y0, x1, y1) in tiles:
        n = (x1 - x0) * (y1 - y0)
        frame[y0:y1, x0:x1] = packed[pos:pos + n].reshape(y1 - y0, x1 - x0, channels)
        pos += n
    return frame


def span_pixels(width, height, rank, world, tile=TILE):
    """Pixels in rank's packed span (the sum of its tiles' areas)."""
    return sum((t[2] - t[0]) * (t[3] - t[1]) for t in tiles_for_rank(width, height, rank, world, tile))


class FrameGather:
    """Multi-GPU exchange.  Every rank holds its tiles' packed span — float linear
    RGB [npx, 3] (the F7 float buffer) or the RGBA8 FrameBuffer bytes [npx, 4] uint8 (what the
    reference's Render writes, Integrator.cpp:327-344) — as a torch tensor on its device, or on
    the CPU under gloo.  One `gather` brings the spans to rank 0 (RCCL over xGMI under the nccl
    backend), padded to the largest span, and rank 0 scatters them into a row-major
    [height*width, channels] frame on its own device (index_copy_ with per-rank pixel indices
    computed once)."""

    def __init__(self, width, height, world, device, tile=TILE, channels=3, dtype=None):
        import torch
        dtype = torch.float32 if dtype is None else dtype
        self.world = world
        self.npx = [span_pixels(width, height, r, world, tile) for r in range(world)]
        self.max_px = max(self.npx)
        self.index = []
        for r in range(world):
            idx = [y * width + x for (x0, y0, x1, y1) in tiles_for_rank(width, height, r, world, tile)
                   for y in range(y0, y1) for x in range(x0, x1)]
            self.index.append(torch.tensor(idx, dtype=torch.long, device=device))
        self.send = torch.zeros((self.max_px, channels), dtype=dtype, device=device)
        self.recv = [torch.empty_like(self.send) for _ in range(world)]
        self.frame = torch.zeros((height * width, channels), dtype=dtype, device=device)

    def __call__(self, span, rank, group=None):
        import torch.distributed as dist
        self.send[:span.shape[0]].copy_(span)
        dist.gather(self.send, gather_list=self.recv if rank == 0 else None, dst=0, group=group)
        if rank != 0:
            return None
        for r in range(self.world):
            self.frame.index_copy_(0, self.index[r], self.recv[r][:self.npx[r]])
        return self.frame


def gather_frame(span, width, height, rank, world, group=None, tile=TILE):
    """One-shot FrameGather: the assembled [height, width, channels] numpy frame on rank 0, None elsewhere."""
    ch = span.shape[1]
    g = FrameGather(width, height, world, span.device, tile, channels=ch, dtype=span.dtype)
    f = g(span, rank, group)
    return None if f is None else f.cpu().numpy().reshape(height, width, ch)
