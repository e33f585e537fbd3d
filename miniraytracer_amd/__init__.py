"""miniraytracer_amd -- MI355X (gfx950) render path for MiniRayTracer scenes.

Host-side mirror of the reference's render interface (the names follow the reference):

* ``ParseArgv(argv)`` / ``MRT_Params``      -- cmdline_parser.cpp:78-107, cmdline_parser.h:5-18
* ``select_scene(scene, aspect)``           -- scene.cpp:25-49 (scenes 0-8, plus 9 = C3 teapot)
* ``Renderer(scene).render(...)``           -- the draw()/draw2() workers over work_queue
                                               (main.cpp:138-243, 347-382), on the GPU
* ``tonemap_argb(img)``                     -- Drago tone map + ARGB32 (main.cpp:416-444)

Everything above the C-ABI is a thin ctypes layer; the render path itself is libmrt.so
(hand-written HIP for gfx950).  No CPU fallback exists.
"""
import ctypes as C
import json
import os

import numpy as np

from . import _lib
from ._lib import MrtError, MrtParams, MrtRenderDesc, MrtSceneView, check, lib

SCENES = ["SCENE_RANDOM_SPHERES", "SCENE_RANDOM_SPHERES_2", "SCENE_TWO_SPHERES", "SCENE_PERLIN_SPHERES",
          "SCENE_EARTH", "SCENE_CORNELL_BOX", "SCENE_CORNELL_SMOKE", "SCENE_BOOK2_FINAL", "SCENE_TRIANGLES",
          "SCENE_TEAPOT_CORNELL"]
MAIN_SEED = 11350390909718046443  # main.cpp:302
ASSET_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")


# mrt_ray / mrt_hit (include/mrt.h "ray queries"), byte for byte
RAY_DTYPE = np.dtype([("o", "<f4", (3,)), ("time", "<f4"), ("d", "<f4", (3,)), ("tmax", "<f4"), ("inside", "<u4"), ("reserved", "<u4", (3,))])
HIT_DTYPE = np.dtype([("t", "<f4"), ("p", "<f4", (3,)), ("n", "<f4", (3,)), ("mat", "<u4")])
NO_HIT = _lib.NO_HIT
assert RAY_DTYPE.itemsize == 48 and HIT_DTYPE.itemsize == 32


def _as_rays(rays):
    """A contiguous RAY_DTYPE array from a RAY_DTYPE array or a float32 (n, 8) array of
    o, time, d, tmax (inside = 0)."""
    a = np.asarray(rays)
    if a.dtype == RAY_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != 8:
        raise ValueError("rays: a RAY_DTYPE array or a float32 (n, 8) array of o, time, d, tmax")
    out = np.zeros(a.shape[0], dtype=RAY_DTYPE)
    out.view(np.float32).reshape(-1, 12)[:, :8] = a
    return out


def camera_pixel_rays(cam, width, height, xs, ys):
    """mrt_camera_pixel_ray (include/mrt.h) for each (xs[k], ys[k]): the pinhole rays through those
    pixel centres under the MrtCamera `cam` (row 0 = bottom), a RAY_DTYPE array with tmax = +inf."""
    xs = np.asarray(xs, dtype=np.int64).reshape(-1)
    ys = np.asarray(ys, dtype=np.int64).reshape(-1)
    if xs.size != ys.size:
        raise ValueError("camera_pixel_rays: xs and ys differ in length")
    if ((xs < 0) | (ys < 0) | (xs >= 2 ** 32) | (ys >= 2 ** 32)).any():
        raise ValueError("camera_pixel_rays: a pixel coordinate outside uint32")
    out = np.zeros(xs.size, dtype=RAY_DTYPE)
    fn, base = lib().mrt_camera_pixel_ray, out.ctypes.data
    for k in range(xs.size):
        check(fn(C.byref(cam), width, height, int(xs[k]), int(ys[k]), C.c_void_p(base + 48 * k)), "mrt_camera_pixel_ray")
    return out


def _range_args(what, first, n):
    first, n = int(first), int(n)
    if first < 0 or first > _U64 or n < 0 or n >= 2 ** 32:
        raise ValueError(f"{what}: first outside uint64 or n outside uint32")
    return first, n


def camera_pixel_ray_range(cam, width, height, first, n):
    """mrt_camera_pixel_rays (include/mrt.h): the pinhole rays through the centres of pixels
    first .. first + n - 1 (row-major, row 0 = bottom) in one call, a RAY_DTYPE array; record j equals
    camera_pixel_rays' ray of pixel first + j."""
    first, n = _range_args("camera_pixel_ray_range", first, n)
    out = np.zeros(n, dtype=RAY_DTYPE)
    check(lib().mrt_camera_pixel_rays(C.byref(cam), width, height, first, n, C.c_void_p(out.ctypes.data)), "mrt_camera_pixel_rays")
    return out


def camera_pixel_rays_device(cam, width, height, first, n, d_out_ptr, stream_ptr=0):
    """The same into device records (a torch data_ptr() of n mrt_ray, 16-byte aligned), enqueued on a
    HIP stream: nothing synchronised, nothing allocated (capturable; the camera is captured by value)."""
    check(lib().mrt_camera_pixel_rays_device(C.byref(cam), width, height, int(first), int(n), C.c_void_p(d_out_ptr or None), C.c_void_p(stream_ptr)),
          "mrt_camera_pixel_rays_device")


# mrt_probe / mrt_radiance (include/mrt.h "radiance queries"), byte for byte
PROBE_DTYPE = np.dtype([("o", "<f4", (3,)), ("time", "<f4"), ("d", "<f4", (3,)), ("inside", "<u4"), ("rng_state", "<u8"), ("rng_inc", "<u8")])
RADIANCE_DTYPE = np.dtype([("L", "<f4", (3,)), ("rays", "<u4")])
assert PROBE_DTYPE.itemsize == 48 and RADIANCE_DTYPE.itemsize == 16
_U64 = 2 ** 64 - 1


def probe_seed(seed, path_id):
    """mrt_probe_seed (include/mrt.h): the (rng_state, rng_inc) words of the render's stream for path_id
    under `seed`, as pcg32_srandom(splitmix64(seed ^ path_id), path_id) leaves them."""
    p = np.zeros(1, dtype=PROBE_DTYPE)
    lib().mrt_probe_seed(C.c_uint64(int(seed) & _U64), C.c_uint64(int(path_id) & _U64), C.c_void_p(p.ctypes.data))
    return int(p["rng_state"][0]), int(p["rng_inc"][0])


def _path_probes(fn, what, first, desc, pixels, samples):
    px, sm = np.broadcast_arrays(np.asarray(pixels, dtype=np.int64), np.asarray(samples, dtype=np.int64))
    px, sm = px.reshape(-1), sm.reshape(-1)
    if ((px < 0) | (sm < 0) | (px >= 2 ** 32) | (sm >= 2 ** 32)).any():
        raise ValueError(f"{what}: a pixel or sample outside uint32")
    out = np.zeros(px.size, dtype=PROBE_DTYPE)
    base = out.ctypes.data
    for k in range(px.size):
        check(fn(C.byref(first), C.byref(desc), int(px[k]), int(sm[k]), C.c_void_p(base + 48 * k)), what)
    return out


def camera_path_probes(cam, desc, pixels, samples):
    """mrt_camera_path_probe (include/mrt.h) for each (pixels[k], samples[k]) (broadcast against each
    other): the starts of the render's paths under the MrtCamera `cam` and `desc` -- origin,
    un-normalised direction, time and the stream after the camera's draws -- as a PROBE_DTYPE array.
    Renderer.trace_rays of them at desc's depth is the render's paths."""
    return _path_probes(lib().mrt_camera_path_probe, "mrt_camera_path_probe", cam, desc, pixels, samples)


def pano_probes(params, desc, pixels, samples):
    """mrt_pano_probe (include/mrt.h): the same grid and keying for an equirectangular camera at
    params.pos (an MrtCameraParams: 360 x 180 degrees, the image centre looks at lookat, up is up)."""
    return _path_probes(lib().mrt_pano_probe, "mrt_pano_probe", params, desc, pixels, samples)


def camera_path_probe_range(cam, desc, first, n):
    """mrt_camera_path_probes (include/mrt.h): the starts of paths first .. first + n - 1 of the render
    `desc` under the MrtCamera `cam`, counted pixel-major (pixel = q // ns, sample = q % ns), in one
    call: a PROBE_DTYPE array whose record j equals camera_path_probes' record of that (pixel, sample)."""
    first, n = _range_args("camera_path_probe_range", first, n)
    out = np.zeros(n, dtype=PROBE_DTYPE)
    check(lib().mrt_camera_path_probes(C.byref(cam), C.byref(desc), first, n, C.c_void_p(out.ctypes.data)), "mrt_camera_path_probes")
    return out


def camera_path_probes_device(cam, desc, first, n, d_out_ptr, stream_ptr=0):
    """The same into device records (a torch data_ptr() of n mrt_probe, 16-byte aligned), enqueued on a
    HIP stream: nothing synchronised, nothing allocated (capturable; cam and desc are captured by value)."""
    check(lib().mrt_camera_path_probes_device(C.byref(cam), C.byref(desc), int(first), int(n), C.c_void_p(d_out_ptr or None), C.c_void_p(stream_ptr)),
          "mrt_camera_path_probes_device")


def pano_probe_range(params, desc, first, n):
    """mrt_pano_probes (include/mrt.h): the same range for the equirectangular camera of pano_probes."""
    first, n = _range_args("pano_probe_range", first, n)
    out = np.zeros(n, dtype=PROBE_DTYPE)
    check(lib().mrt_pano_probes(C.byref(params), C.byref(desc), first, n, C.c_void_p(out.ctypes.data)), "mrt_pano_probes")
    return out


def pano_probes_device(params, desc, first, n, d_out_ptr, stream_ptr=0):
    """The same into device records, enqueued on a HIP stream (as camera_path_probes_device)."""
    check(lib().mrt_pano_probes_device(C.byref(params), C.byref(desc), int(first), int(n), C.c_void_p(d_out_ptr or None), C.c_void_p(stream_ptr)),
          "mrt_pano_probes_device")


def surface_probes(hits, rays=None, sqrt_per_hit=1, seed=0, first_id=0):
    """mrt_surface_probes (include/mrt.h): sqrt_per_hit^2 cosine-distributed probes leaving the point of
    each HIT_DTYPE record (Renderer.cast_rays' output), stratified on a jittered grid, from the streams
    keyed by first_id + j under `seed` -- a PROBE_DTYPE array, hit-major.  rays (the RAY_DTYPE records
    that were cast, optional) turn each normal towards its ray and give the probes its time.  A miss
    (mat == NO_HIT) gives a null record: mask by mat.  pi * mean(L) over a hit's probes estimates the
    irradiance there."""
    h = np.asarray(hits)
    if h.dtype != HIT_DTYPE:
        raise ValueError("surface_probes: hits must be a HIT_DTYPE array")
    h = np.ascontiguousarray(h).reshape(-1)
    r = None
    if rays is not None:
        r = _as_rays(rays)
        if r.size != h.size:
            raise ValueError("surface_probes: rays and hits differ in length")
    sq = int(sqrt_per_hit)
    if sq < 0 or sq >= 2 ** 32:
        raise ValueError("surface_probes: sqrt_per_hit outside uint32")
    total = h.size * sq * sq
    out = np.zeros(total if total < 2 ** 32 else 0, dtype=PROBE_DTYPE)
    check(lib().mrt_surface_probes(C.c_void_p(h.ctypes.data), C.c_void_p(r.ctypes.data if r is not None else None), h.size, sq,
                                   int(seed) & _U64, int(first_id) & _U64, C.c_void_p(out.ctypes.data)), "mrt_surface_probes")
    return out


def surface_probes_device(d_hits_ptr, d_rays_ptr, n_hits, d_out_ptr, sqrt_per_hit=1, seed=0, first_id=0, stream_ptr=0):
    """The same on device records (torch data_ptr()s of n_hits mrt_hit, n_hits mrt_ray or 0, and
    n_hits * sqrt_per_hit^2 mrt_probe, 16-byte aligned), enqueued on a HIP stream: nothing synchronised,
    nothing allocated (capturable: a replay reads whatever the hit records then hold)."""
    check(lib().mrt_surface_probes_device(C.c_void_p(d_hits_ptr or None), C.c_void_p(d_rays_ptr or None), int(n_hits), int(sqrt_per_hit),
                                          int(seed) & _U64, int(first_id) & _U64, C.c_void_p(d_out_ptr or None), C.c_void_p(stream_ptr)),
          "mrt_surface_probes_device")


def _as_radiance(rad, group):
    a = np.asarray(rad)
    if a.dtype != RADIANCE_DTYPE:
        raise ValueError("radiance_fold: a RADIANCE_DTYPE array")
    a = np.ascontiguousarray(a).reshape(-1)
    if group < 1 or a.size % group:
        raise ValueError("radiance_fold: the records must be whole groups")
    return a


def radiance_fold(rad, group, max_luminance=1000.0):
    """mrt_radiance_fold (include/mrt.h) on the host: draw()'s pixel over each `group` consecutive
    RADIANCE_DTYPE records -- the sum in record order with the NaN rule, divided by group, clamped to
    max_luminance -- as a float32 (n / group, 4) array (w = 0)."""
    a = _as_radiance(rad, group)
    out = np.zeros((a.size // group, 4), dtype=np.float32)
    check(lib().mrt_radiance_fold(C.c_void_p(a.ctypes.data), a.size // group, group, max_luminance, C.c_void_p(out.ctypes.data)), "mrt_radiance_fold")
    return out


def radiance_fold_device(d_rad_ptr, n_groups, group, d_rgb_ptr, max_luminance=1000.0, stream_ptr=0):
    """The same on device records (torch data_ptr()s: n_groups * group mrt_radiance, n_groups float4,
    16-byte aligned), enqueued on a HIP stream."""
    check(lib().mrt_radiance_fold_device(C.c_void_p(d_rad_ptr or None), n_groups, group, max_luminance, C.c_void_p(d_rgb_ptr or None),
                                         C.c_void_p(stream_ptr)), "mrt_radiance_fold_device")


def radiance_rays_device(d_rad_ptr, n, d_rays_ptr, stream_ptr=0):
    """mrt_radiance_rays_device (include/mrt.h): adds the ray counts of n device RADIANCE records to the
    device uint64 at d_rays_ptr (zeroed by the caller), enqueued on a HIP stream."""
    check(lib().mrt_radiance_rays_device(C.c_void_p(d_rad_ptr or None), int(n), C.c_void_p(d_rays_ptr or None), C.c_void_p(stream_ptr)),
          "mrt_radiance_rays_device")


def default_params():
    p = MrtParams()
    lib().mrt_default_params(C.byref(p))
    return p


def ParseArgv(argv):
    """Parse reference command-line flags (argv[0] is the program name)."""
    p = MrtParams()
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    st = lib().mrt_parse_argv(len(argv), arr, C.byref(p))
    if st != 0:
        raise SystemExit(0)  # -help
    return p


class Scene:
    """Host-side scene built by select_scene (the flattened scene blob)."""

    def __init__(self, handle, scene_id):
        self._h = C.c_void_p(handle)
        self.scene_id = scene_id
        self.view = MrtSceneView()
        check(lib().mrt_scene_blob_view(self._h, C.byref(self.view)), "mrt_scene_blob_view")

    def dump_json(self):
        out = C.c_void_p()
        check(lib().mrt_scene_blob_dump_json(self._h, C.byref(out)), "dump")
        try:
            return json.loads(C.cast(out, C.c_char_p).value.decode())
        finally:
            lib().mrt_free_string(out)

    def worker_seeds(self, n_threads):
        """[(initstate, initseq)] main() gives its worker threads (main.cpp:357-361)."""
        a = np.zeros(n_threads, dtype=np.uint64)
        b = np.zeros(n_threads, dtype=np.uint64)
        check(lib().mrt_worker_seeds(self._h, n_threads, a.ctypes.data, b.ctypes.data), "mrt_worker_seeds")
        return [(int(x), int(y)) for x, y in zip(a, b)]

    def camera_params(self):
        """The mrt_camera_params the scene's builder used (position, look-at, up, vfov_deg, aspect,
        aperture, focus_dist, time0, time1): make_camera(scene.camera_params()) is scene.view.camera."""
        p = _lib.MrtCameraParams()
        check(lib().mrt_scene_camera_params(self._h, C.byref(p)), "mrt_scene_camera_params")
        return p

    def close(self):
        if self._h:
            lib().mrt_scene_blob_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def select_scene(scene, aspect, asset_dir=None):
    h = C.c_void_p()
    ad = (asset_dir or os.environ.get("MRT_ASSET_DIR") or ASSET_DIR).encode()
    check(lib().mrt_select_scene(int(scene), float(aspect), ad, C.byref(h)), f"select_scene({scene})")
    return Scene(h.value, scene)


NUMERICS = ("exact", "fast")


def render_desc(width, height, samples, depth=32, max_luminance=1000.0, mode=0, seed=MAIN_SEED, tile_size=32,
                rank=0, world=1, chunk_samples=0, flags=0, numerics="exact", threads=0, preview=False, ref_order=False,
                pixels=None):
    """Render description; `samples` is floored to a perfect square like main.cpp:319-320.
    numerics: "exact" (bit-for-bit the reference built exact) or "fast" (tolerance contract:
    per-pixel RMSE < 1e-3 vs the reference as shipped; MRT_RF_FAST).  ref_order (CPU backend): the
    reference's own RNG order, one stream per worker thread (Renderer.set_worker_seeds).
    pixels: optional row-major pixel indices to render instead of the rank's tiles (the desc keeps
    a reference to the array; mrt_render_desc.pixels)."""
    if numerics not in NUMERICS:
        raise ValueError(f"numerics must be one of {NUMERICS}")
    if numerics == "fast":
        flags |= _lib.RF_FAST
    if preview:
        flags |= _lib.RF_PREVIEW
    if ref_order:
        flags |= _lib.RF_REF_ORDER
    sq = int(np.sqrt(np.float32(samples)))
    d = MrtRenderDesc(width, height, sq, depth, max_luminance, mode, seed, tile_size, rank, world,
                      chunk_samples, flags, threads)
    if pixels is not None:
        px = np.ascontiguousarray(pixels, dtype=np.uint32)
        d.pixels = px.ctypes.data
        d.n_pixels = px.size
        d._pixels = px  # keeps the list alive as long as the desc
    return d


def local_pixels(desc):
    n = C.c_uint32()
    check(lib().mrt_local_pixels(C.byref(desc), C.byref(n), None), "local_pixels")
    px = np.zeros(n.value, dtype=np.uint32)
    check(lib().mrt_local_pixels(C.byref(desc), C.byref(n), px.ctypes.data), "local_pixels")
    return px


def device_count():
    n = C.c_int()
    st = lib().mrt_init(C.byref(n))
    return n.value if st == 0 else 0


class Renderer:
    """A scene resident in HBM of one device -- or, with device="cpu" (MRT_DEVICE_CPU), held by the
    CPU backend: the same hot-path code compiled for the host, exact numerics contract, worker
    threads over the work_queue tiles (render_desc(threads=...)).  Only an explicit "cpu" selects
    it; without a gfx950 device a GPU Renderer raises."""

    def __init__(self, scene, device=0):
        if device == "cpu":
            device = _lib.DEVICE_CPU
        else:
            n = C.c_int()
            check(lib().mrt_init(C.byref(n)), "mrt_init")
        self.device = device
        self._h = C.c_void_p()
        check(lib().mrt_scene_upload(device, C.byref(scene.view), C.byref(self._h)), "mrt_scene_upload")
        self.scene = scene

    def render(self, desc, cancel=None):
        """Blocking render into a host float32 (H, W, 4) image (row 0 = bottom); returns (img, rays).
        cancel: optional ctypes.c_int; setting it non-zero from another thread stops the render
        (G_isRunning, main.cpp:180/235) and raises MrtError (MRT_ERR_CANCELLED)."""
        img = np.zeros((desc.height, desc.width, 4), dtype=np.float32)
        rays = C.c_uint64()
        check(lib().mrt_render(self._h, C.byref(desc), img.ctypes.data, C.byref(rays), C.byref(cancel) if cancel is not None else None),
              "mrt_render")
        return img, rays.value

    def set_worker_seeds(self, seeds):
        """CPU backend: the (initstate, initseq) of each worker thread (main.cpp:357-366, e.g.
        scene.worker_seeds(n)) for renders in the reference's RNG order (render_desc(ref_order=True))."""
        a = np.array([s[0] for s in seeds], dtype=np.uint64)
        b = np.array([s[1] for s in seeds], dtype=np.uint64)
        check(lib().mrt_set_worker_seeds(self._h, len(seeds), a.ctypes.data, b.ctypes.data), "mrt_set_worker_seeds")

    def prepare(self, desc):
        check(lib().mrt_prepare(self._h, C.byref(desc)), "mrt_prepare")

    def render_device(self, desc, d_out_ptr, d_rays_ptr, stream_ptr=0):
        """Enqueue a render into device memory (torch tensor data_ptr()s) on a HIP stream."""
        check(lib().mrt_render_device(self._h, C.byref(desc), C.c_void_p(d_out_ptr), C.c_void_p(d_rays_ptr),
                                      C.c_void_p(stream_ptr)), "mrt_render_device")

    def render_aux(self, desc):
        """First-hit feature buffers of desc's pixels (include/mrt.h mrt_render_aux), both backends:
        (normal, albedo), float32 (H, W, 4) each -- normal = (n.xyz facing the ray, coverage), albedo =
        (r, g, b, depth), the mean over the desc's samples; only owned pixels are written."""
        normal = np.zeros((desc.height, desc.width, 4), dtype=np.float32)
        albedo = np.zeros((desc.height, desc.width, 4), dtype=np.float32)
        check(lib().mrt_render_aux(self._h, C.byref(desc), normal.ctypes.data, albedo.ctypes.data), "mrt_render_aux")
        return normal, albedo

    def render_aux_device(self, desc, d_normal_ptr, d_albedo_ptr, stream_ptr=0):
        """Enqueue the feature buffers into device memory (n_local float4 each, local_pixels order)."""
        check(lib().mrt_render_aux_device(self._h, C.byref(desc), C.c_void_p(d_normal_ptr), C.c_void_p(d_albedo_ptr),
                                          C.c_void_p(stream_ptr)), "mrt_render_aux_device")

    def cast_rays(self, rays, seed=0):
        """Closest hits of caller rays (include/mrt.h mrt_cast_rays), both backends: a HIT_DTYPE array,
        one record per ray -- (t, p, n, mat), or (+inf, 0, 0, NO_HIT) for a miss or a hit past the ray's
        tmax.  rays: a RAY_DTYPE array, or float32 (n, 8) rows of o, time, d, tmax (inside = 0).  Ray i
        draws a volume's random numbers from the stream keyed by seed + i."""
        r = _as_rays(rays)
        hits = np.zeros(r.size, dtype=HIT_DTYPE)
        check(lib().mrt_cast_rays(self._h, C.c_void_p(r.ctypes.data), r.size, C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_void_p(hits.ctypes.data)),
              "mrt_cast_rays")
        return hits

    def cast_rays_device(self, d_rays_ptr, n, d_hits_ptr, seed=0, stream_ptr=0):
        """The same on device records (torch data_ptr()s of n mrt_ray / n mrt_hit, 16-byte aligned),
        enqueued on a HIP stream: nothing synchronised, nothing allocated (capturable)."""
        check(lib().mrt_cast_rays_device(self._h, C.c_void_p(d_rays_ptr or None), n, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                         C.c_void_p(d_hits_ptr or None), C.c_void_p(stream_ptr)), "mrt_cast_rays_device")

    def trace_rays(self, probes, depth=32):
        """Path-traced radiance along caller rays (include/mrt.h mrt_trace_rays), both backends:
        (records, rays) -- a RADIANCE_DTYPE array, one record per probe (L as trace() returns it, the
        path's ray count), and the total of the ray counts.  probes: a PROBE_DTYPE array (e.g.
        camera_path_probes, pano_probes, or your own rays with probe_seed streams)."""
        p = np.asarray(probes)
        if p.dtype != PROBE_DTYPE:
            raise ValueError("probes: a PROBE_DTYPE array")
        p = np.ascontiguousarray(p).reshape(-1)
        out = np.zeros(p.size, dtype=RADIANCE_DTYPE)
        rays = C.c_uint64()
        check(lib().mrt_trace_rays(self._h, C.c_void_p(p.ctypes.data), p.size, depth, C.c_void_p(out.ctypes.data), C.byref(rays)), "mrt_trace_rays")
        return out, rays.value

    def trace_rays_workspace(self, depth=32):
        """(bytes_full, bytes_min) of fold-level storage for trace_rays_device at `depth`: the kernel's
        full grid and one wave (GPU)."""
        full, least = C.c_uint64(), C.c_uint64()
        check(lib().mrt_trace_rays_workspace(self._h, depth, C.byref(full), C.byref(least)), "mrt_trace_rays_workspace")
        return full.value, least.value

    def trace_rays_device(self, d_probes_ptr, n, d_out_ptr, d_work_ptr, work_bytes, depth=32, stream_ptr=0):
        """The same on device records (torch data_ptr()s of n mrt_probe / n mrt_radiance and a workspace
        of work_bytes, all 16-byte aligned), enqueued on a HIP stream: nothing synchronised, nothing
        allocated (capturable).  The grid follows work_bytes (trace_rays_workspace)."""
        check(lib().mrt_trace_rays_device(self._h, C.c_void_p(d_probes_ptr or None), n, depth, C.c_void_p(d_out_ptr or None),
                                          C.c_void_p(d_work_ptr or None), work_bytes, C.c_void_p(stream_ptr)), "mrt_trace_rays_device")

    def render_adaptive(self, desc, params=None, cancel=None):
        """Adaptive render (include/mrt.h mrt_render_adaptive), both backends: desc as the base pass, then
        up to params.max_passes refinement passes over the pixels whose standard error misses
        atol + rtol * mean.  Returns (img, moments, rays): float32 (H, W, 4) each -- moments = (sum l,
        sum l^2, n_finite, samples spent) per pixel -- and the ray total of all passes."""
        p = params if params is not None else default_adaptive_params()
        img = np.zeros((desc.height, desc.width, 4), dtype=np.float32)
        mom = np.zeros((desc.height, desc.width, 4), dtype=np.float32)
        rays = C.c_uint64()
        check(lib().mrt_render_adaptive(self._h, C.byref(desc), C.byref(p), img.ctypes.data, mom.ctypes.data, C.byref(rays),
                                        C.byref(cancel) if cancel is not None else None), "mrt_render_adaptive")
        return img, mom, rays.value

    def set_camera(self, cam, stream_ptr=None):
        """Replace the scene's camera (an MrtCamera, e.g. make_camera(...)); nothing is uploaded again.
        stream_ptr=None: the blocking form (both backends; waits for the scene's pending work).
        Otherwise (GPU): enqueued on that HIP stream (0 = the null stream) -- renders enqueued on it
        earlier see the old camera, later ones the new; capturable; the caller orders it against work on
        other streams (after join() under RF_FOLD_ASYNC)."""
        if stream_ptr is None:
            check(lib().mrt_scene_set_camera(self._h, C.byref(cam)), "mrt_scene_set_camera")
        else:
            check(lib().mrt_scene_set_camera_device(self._h, C.byref(cam), C.c_void_p(stream_ptr)), "mrt_scene_set_camera_device")

    def join(self, stream_ptr=0):
        """Order a HIP stream after this context's last render_device (its fold runs on the context's
        own stream under RF_FOLD_ASYNC): the worker threads' join() (main.cpp:490-493)."""
        check(lib().mrt_render_join(self._h, C.c_void_p(stream_ptr)), "mrt_render_join")

    def preview(self, width, height):
        """The running render as the reference's UI thread sees G_linearBackBuffer (main.cpp:387-444):
        (H, W, 4) float32 image after `samples` samples of every pixel, callable from another thread
        while render() runs.  GPU: renders made with flags=RF_PREVIEW (render_desc(preview=True))."""
        img = np.zeros((height, width, 4), dtype=np.float32)
        n = C.c_uint32()
        check(lib().mrt_preview(self._h, img.ctypes.data, C.byref(n)), "mrt_preview")
        return img, n.value

    def progress(self):
        """Percent of the current / last render's paths handed out (work_queue::getPercentDone)."""
        pct = C.c_float()
        check(lib().mrt_progress(self._h, C.byref(pct)), "mrt_progress")
        return pct.value

    def kernel_info(self):
        """dict(features, kernel_features, lds_bytes, grid, prog_ops) of the path kernel this scene runs."""
        ki = _lib.KernelInfo()
        check(lib().mrt_scene_kernel_info(self._h, C.byref(ki)), "mrt_scene_kernel_info")
        return {k: getattr(ki, k) for k, _ in ki._fields_}

    def kernel_ms(self):
        """(total ms, launches) of the path kernel in the last render (HIP events on its stream)."""
        ms, n = C.c_float(), C.c_uint32()
        check(lib().mrt_kernel_ms(self._h, C.byref(ms), C.byref(n)), "mrt_kernel_ms")
        return ms.value, n.value

    def paths(self, n_paths):
        """Per-path radiance and ray counts of the last MRT_RF_PATH_DEBUG render ([s][local pixel])."""
        rgb = np.zeros((n_paths, 3), dtype=np.float32)
        rays = np.zeros(n_paths, dtype=np.uint32)
        check(lib().mrt_render_debug(self._h, rgb.ctypes.data, rays.ctypes.data, n_paths), "mrt_render_debug")
        return rgb, rays

    def close(self):
        if self._h:
            lib().mrt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    """ncclGetUniqueId for mrt_comm_init_rank (rank 0 makes it, the others receive it out of band)."""
    buf = (C.c_uint8 * _lib.COMM_ID_BYTES)()
    check(lib().mrt_comm_unique_id(buf), "mrt_comm_unique_id")
    return bytes(buf)


def gather_shard_pixels(desc):
    """Pixels of the largest rank shard of desc's tile deal (the RCCL gather's padded shard)."""
    n = C.c_uint32()
    check(lib().mrt_gather_shard_pixels(C.byref(desc), C.byref(n)), "mrt_gather_shard_pixels")
    return n.value


class Comm:
    """One rank of an RCCL communicator for the framebuffer gather (include/mrt.h "multi-GPU"):
    Comm(device, world, rank, uid) per process (mrt_comm_init_rank), or Comm.init_all(devices) for one
    process driving every GPU (mrt_comm_init_all)."""

    def __init__(self, device=0, world=1, rank=0, uid=None, _handle=None):
        self.device, self.world, self.rank = device, world, rank
        self._h = C.c_void_p(_handle)
        if _handle is None:
            buf = (C.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(uid if uid is not None else comm_unique_id())
            check(lib().mrt_comm_init_rank(device, world, rank, buf, C.byref(self._h)), "mrt_comm_init_rank")

    @classmethod
    def init_all(cls, devices):
        n = len(devices)
        devs = (C.c_int * n)(*devices)
        hs = (C.c_void_p * n)()
        check(lib().mrt_comm_init_all(n, devs, hs), "mrt_comm_init_all")
        return [cls(devices[r], n, r, _handle=hs[r]) for r in range(n)]

    def gather_frame(self, desc, d_local_ptr, d_frame_ptr, d_rays_ptr=0, stream_ptr=0):
        """Collective: this rank's shard (render_device output) to the root's W*H float4 frame, rays
        all-reduced in place (device pointers, e.g. torch data_ptr()s; enqueued on a HIP stream)."""
        check(lib().mrt_gather_frame(self._h, C.byref(desc), C.c_void_p(d_local_ptr), C.c_void_p(d_frame_ptr or None),
                                     C.c_void_p(d_rays_ptr or None), C.c_void_p(stream_ptr)), "mrt_gather_frame")

    def render_gather(self, renderer, desc):
        """Collective render + RCCL gather: the whole (H, W, 4) image on the root (None elsewhere) and
        the ray total of all ranks."""
        img = np.zeros((desc.height, desc.width, 4), dtype=np.float32) if self.rank == 0 else None
        rays = C.c_uint64()
        check(lib().mrt_render_gather(renderer._h, self._h, C.byref(desc), img.ctypes.data if img is not None else None,
                                      C.byref(rays)), "mrt_render_gather")
        return img, rays.value

    def close(self):
        if self._h:
            lib().mrt_comm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tonemap_device(d_rgb_ptr, n, d_lwmax_ptr, d_argb_ptr, stream_ptr=0, reduce=True):
    """Device tone map of n float4 pixels (torch data_ptr()s).  reduce=True first max-reduces the
    luminance into *d_lwmax (which the caller zeroed); pass reduce=False after combining L_wmax
    across ranks yourself."""
    if reduce:
        check(lib().mrt_lum_max_device(C.c_void_p(d_rgb_ptr), n, C.c_void_p(d_lwmax_ptr), C.c_void_p(stream_ptr)), "mrt_lum_max_device")
    check(lib().mrt_tonemap_device(C.c_void_p(d_rgb_ptr), n, C.c_void_p(d_lwmax_ptr), C.c_void_p(d_argb_ptr), C.c_void_p(stream_ptr)),
          "mrt_tonemap_device")


MATHFN = ("sin", "cos", "tan", "log", "log10", "asin", "exp", "pow5", "atan2", "pow")  # include/mrt.h MRT_FN_*
MATHFN_D = ("sincos", "log", "exp", "atan2")  # include/mrt.h MRT_FND_*


def _fn_index(names, name):
    if name not in names:
        raise ValueError(f"mathfn: unknown function {name!r} (one of {', '.join(names)})")
    return names.index(name)


def mathfn(name, a, b=None):
    """The numerics contract's float function `name` of MATHFN (include/mrt_mathfn.h) over float32
    arrays on the host: f(a), atan2(a, b), pow(a, b)."""
    w = _fn_index(MATHFN, name)
    a = np.ascontiguousarray(a, dtype=np.float32)
    if w >= 8:
        if b is None:
            raise ValueError(f"mathfn: {name} takes two arrays")
        b = np.ascontiguousarray(b, dtype=np.float32)
        if b.shape != a.shape:
            raise ValueError("mathfn: a and b must have one shape")
    out = np.zeros(a.shape, dtype=np.float32)
    check(lib().mrt_mathfn(w, a.size, a.ctypes.data, b.ctypes.data if w >= 8 else None, out.ctypes.data), "mrt_mathfn")
    return out


def mathfn_device(name, n, a_ptr, b_ptr, out_ptr, stream=0):
    """The same on the device (torch data_ptr()s of n floats each; b_ptr may be 0 for the one-argument
    functions), enqueued on a HIP stream: one thread per element, exactly n results."""
    check(lib().mrt_mathfn_device(_fn_index(MATHFN, name), n, C.c_void_p(a_ptr or None), C.c_void_p(b_ptr or None), C.c_void_p(out_ptr or None),
                                  C.c_void_p(stream)), "mrt_mathfn_device")


def mathfn_d(name, a, b=None):
    """The double core `name` of MATHFN_D (mrt_sincos_d, mrt_log_d, mrt_exp_d, mrt_atan2_d(a, b)) over
    float64 arrays on the host; "sincos" returns (sin, cos)."""
    w = _fn_index(MATHFN_D, name)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if w == 3:
        if b is None:
            raise ValueError("mathfn_d: atan2 takes two arrays")
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != a.shape:
            raise ValueError("mathfn_d: a and b must have one shape")
    out = np.zeros(a.shape, dtype=np.float64)
    out2 = np.zeros(a.shape, dtype=np.float64) if w == 0 else None
    check(lib().mrt_mathfn_d(w, a.size, a.ctypes.data, b.ctypes.data if w == 3 else None, out.ctypes.data,
                             out2.ctypes.data if w == 0 else None), "mrt_mathfn_d")
    return (out, out2) if w == 0 else out


def mathfn_d_device(name, n, a_ptr, b_ptr, out_ptr, out2_ptr=0, stream=0):
    """The same on the device (torch data_ptr()s of n doubles each; out2_ptr receives "sincos"'s cosines
    and may be 0 otherwise, b_ptr may be 0 but for "atan2"), enqueued on a HIP stream."""
    check(lib().mrt_mathfn_d_device(_fn_index(MATHFN_D, name), n, C.c_void_p(a_ptr or None), C.c_void_p(b_ptr or None), C.c_void_p(out_ptr or None),
                                    C.c_void_p(out2_ptr or None), C.c_void_p(stream)), "mrt_mathfn_d_device")


def default_denoise_params():
    """mrt_denoise_params with the library's defaults (iterations, sigma_color, sigma_normal,
    sigma_albedo, sigma_depth)."""
    p = _lib.MrtDenoiseParams()
    lib().mrt_default_denoise_params(C.byref(p))
    return p


def denoise(img, normal, albedo, params=None):
    """Edge-avoiding a-trous filter (include/mrt_denoise.h) of a host (H, W, 4) float32 image with
    its feature buffers (Renderer.render_aux); returns the filtered (H, W, 4) image."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    albedo = np.ascontiguousarray(albedo, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 4 or normal.shape != img.shape or albedo.shape != img.shape:
        raise ValueError("denoise: img, normal and albedo must be (H, W, 4) arrays of one shape")
    p = params if params is not None else default_denoise_params()
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    check(lib().mrt_denoise(img.ctypes.data, normal.ctypes.data, albedo.ctypes.data, w, h, C.byref(p), out.ctypes.data), "mrt_denoise")
    return out


def denoise_device(d_rgb_ptr, d_normal_ptr, d_albedo_ptr, width, height, d_out_ptr, d_tmp_ptr, params=None, stream_ptr=0):
    """The same filter on whole row-major device frames (W*H float4 each, torch data_ptr()s), enqueued
    on a HIP stream: the result lands in d_out; d_tmp is scratch; d_rgb is not written."""
    p = params if params is not None else default_denoise_params()
    check(lib().mrt_denoise_device(C.c_void_p(d_rgb_ptr), C.c_void_p(d_normal_ptr), C.c_void_p(d_albedo_ptr), width, height,
                                   C.byref(p), C.c_void_p(d_out_ptr), C.c_void_p(d_tmp_ptr), C.c_void_p(stream_ptr)), "mrt_denoise_device")


def default_adaptive_params(max_passes=None, atol=None, rtol=None):
    """mrt_adaptive_params with the library's defaults (max_passes, atol, rtol), overridden where given."""
    p = _lib.MrtAdaptiveParams()
    lib().mrt_default_adaptive_params(C.byref(p))
    if max_passes is not None:
        p.max_passes = max_passes
    if atol is not None:
        p.atol = atol
    if rtol is not None:
        p.rtol = rtol
    return p


def moments(path_rgb, n_pixels, n_samples, slots=None, out=None):
    """Per-pixel sample moments (include/mrt.h mrt_moments) of per-path radiance in the render's
    layout ([s][local pixel] float3, as Renderer.paths returns it), on the host: (sum l, sum l^2,
    n_finite, samples) per slot, slot = slots[local pixel] (no repeats) or the local pixel itself.
    out: float32 (n, 4) moments to accumulate onto (returned); default zeros for n_pixels slots."""
    rgb = np.ascontiguousarray(path_rgb, dtype=np.float32)
    if rgb.size != n_pixels * n_samples * 3:
        raise ValueError("moments: path_rgb must hold n_samples * n_pixels * 3 floats")
    sl = None
    if slots is not None:
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        if sl.size != n_pixels or len(np.unique(sl)) != n_pixels:
            raise ValueError("moments: slots must hold n_pixels distinct indices")
    if out is None:
        out = np.zeros((n_pixels if sl is None else max(n_pixels, int(sl.max()) + 1), 4), dtype=np.float32)
    if out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"] or out.size < 4 * (n_pixels if sl is None else int(sl.max()) + 1):
        raise ValueError("moments: out must be a contiguous float32 array of (slots, 4)")
    check(lib().mrt_moments(rgb.ctypes.data, n_pixels, n_samples, sl.ctypes.data if sl is not None else None, out.ctypes.data), "mrt_moments")
    return out


def moments_device(d_path_rgb_ptr, n_pixels, n_samples, d_moments_ptr, d_slots_ptr=0, stream_ptr=0):
    """The same on the device (torch data_ptr()s), enqueued on a HIP stream: the chunk's samples are
    added to the float4 moments at d_moments (zeroed by the caller before the first call)."""
    check(lib().mrt_moments_device(C.c_void_p(d_path_rgb_ptr), n_pixels, n_samples, C.c_void_p(d_slots_ptr or None), C.c_void_p(d_moments_ptr),
                                   C.c_void_p(stream_ptr)), "mrt_moments_device")


def moments_se(moments):
    """Standard error of each pixel's mean luminance from its moments (..., 4): a numpy restatement of
    include/mrt_adaptive.h's mrt_moments_se in float32 -- +inf below two finite samples."""
    m = np.asarray(moments, dtype=np.float32)
    sx, sy, n = m[..., 0], m[..., 1], m[..., 2]
    with np.errstate(all="ignore"):
        mean = sx / n
        var = sy / n - mean * mean
        var = np.where(var < 0, np.float32(0), var)
        se = np.sqrt(var / (n - np.float32(1)))
    return np.where(n < 2, np.float32(np.inf), se).astype(np.float32)


def moments_refine(moments, atol, rtol):
    """The adaptive render's own decision (mrt_moments_decide, the library's mrt_moments_refine) for
    float32 moments (..., 4): a bool array, True where the pixel refines."""
    m = np.ascontiguousarray(moments, dtype=np.float32)
    out = np.zeros(m.shape[:-1], dtype=np.uint8)
    check(lib().mrt_moments_decide(m.ctypes.data, out.size, atol, rtol, out.ctypes.data, None), "mrt_moments_decide")
    return out.astype(bool)


def make_camera(params=None, **kw):
    """mrt_make_camera (include/mrt.h): the MrtCamera of camera parameters -- an MrtCameraParams (e.g.
    scene.camera_params()), with fields overridden by keywords: pos, lookat, up (3 floats each),
    vfov_deg, aspect, aperture, focus_dist, time0, time1.  Raises MrtError for a degenerate frame."""
    p = _lib.MrtCameraParams()
    if params is not None:
        C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
    elif not {"pos", "lookat", "vfov_deg", "focus_dist"} <= set(kw):
        raise ValueError("make_camera: without params, give at least pos, lookat, vfov_deg and focus_dist")
    else:
        p.up[:] = (0.0, 1.0, 0.0)
        p.aspect, p.time0, p.time1 = 1.0, 0.0, 1.0
    for k, v in kw.items():
        if k in ("pos", "lookat", "up"):
            getattr(p, k)[:] = [float(x) for x in v]
        elif k in ("vfov_deg", "aspect", "aperture", "focus_dist", "time0", "time1"):
            setattr(p, k, float(v))
        else:
            raise TypeError(f"make_camera: unknown parameter {k}")
    cam = _lib.MrtCamera()
    check(lib().mrt_make_camera(C.byref(p), C.byref(cam)), "mrt_make_camera")
    return cam


def default_temporal_params(**kw):
    """mrt_temporal_params with the library's defaults (max_history, normal_min, depth_tol, albedo_tol,
    min_weight), overridden where given."""
    p = _lib.MrtTemporalParams()
    lib().mrt_default_temporal_params(C.byref(p))
    for k, v in kw.items():
        if k not in dict(p._fields_):
            raise TypeError(f"default_temporal_params: unknown parameter {k}")
        setattr(p, k, v)
    return p


def reproject(img, normal, albedo, cam, hist=None, prev_normal=None, prev_albedo=None, prev_cam=None, params=None):
    """Temporal reprojection on the host (include/mrt_temporal.h): the new history frame (H, W, 4) --
    (accumulated rgb, history length) -- from the current colour and feature buffers under `cam` and
    the previous history frame with the feature buffers and camera it was made with.  hist=None is
    the first frame: (img.xyz, 1)."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    fr = [np.ascontiguousarray(a, dtype=np.float32) for a in (normal, albedo)]
    if hist is not None:
        if prev_normal is None or prev_albedo is None or prev_cam is None:
            raise ValueError("reproject: a history frame needs prev_normal, prev_albedo and prev_cam")
        fr += [np.ascontiguousarray(a, dtype=np.float32) for a in (hist, prev_normal, prev_albedo)]
    if img.ndim != 3 or img.shape[2] != 4 or any(a.shape != img.shape for a in fr):
        raise ValueError("reproject: every frame must be an (H, W, 4) array of one shape")
    p = params if params is not None else default_temporal_params()
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    prev = [a.ctypes.data for a in fr[2:]] if hist is not None else [None, None, None]
    check(lib().mrt_reproject(img.ctypes.data, fr[0].ctypes.data, fr[1].ctypes.data, C.byref(cam), *prev,
                              C.byref(prev_cam) if hist is not None else None, w, h, C.byref(p), out.ctypes.data), "mrt_reproject")
    return out


def reproject_device(d_rgb_ptr, d_normal_ptr, d_albedo_ptr, cam, width, height, d_out_ptr, d_hist_ptr=0, d_prev_normal_ptr=0,
                     d_prev_albedo_ptr=0, prev_cam=None, params=None, stream_ptr=0):
    """The same on whole row-major device frames (W*H float4 each, torch data_ptr()s), enqueued on a
    HIP stream: the new history frame lands in d_out (none of the inputs; they are not written).
    d_hist_ptr=0 is the first frame."""
    p = params if params is not None else default_temporal_params()
    check(lib().mrt_reproject_device(C.c_void_p(d_rgb_ptr), C.c_void_p(d_normal_ptr), C.c_void_p(d_albedo_ptr), C.byref(cam),
                                     C.c_void_p(d_hist_ptr or None), C.c_void_p(d_prev_normal_ptr or None), C.c_void_p(d_prev_albedo_ptr or None),
                                     C.byref(prev_cam) if prev_cam is not None else None, width, height, C.byref(p), C.c_void_p(d_out_ptr),
                                     C.c_void_p(stream_ptr)), "mrt_reproject_device")


def tonemap_argb(img):
    img = np.ascontiguousarray(img, dtype=np.float32)
    h, w = img.shape[:2]
    out = np.zeros((h, w), dtype=np.uint32)
    check(lib().mrt_tonemap_argb(img.ctypes.data, w, h, out.ctypes.data), "tonemap")
    return out


def write_pfm(path, img):
    """Linear PFM, rows bottom-to-top (the PFM convention == G_linearBackBuffer order)."""
    h, w = img.shape[:2]
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(img[..., :3], dtype="<f4").tobytes())


def read_pfm(path):
    with open(path, "rb") as f:
        data = f.read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], dtype="<f4").reshape(h, w, 3)


def write_ppm(path, argb):
    """Tone-mapped 8-bit PPM, displayed top row first (SDL_FLIP_VERTICAL, platform_linux.cpp:84)."""
    h, w = argb.shape
    rgb = np.stack([(argb >> 16) & 255, (argb >> 8) & 255, argb & 255], axis=-1).astype(np.uint8)[::-1]
    with open(path, "wb") as f:
        f.write(f"P6\n{w} {h}\n255\n".encode())
        f.write(rgb.tobytes())
