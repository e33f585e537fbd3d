"""Device cost of the ray queries (DESIGN.md "Ray queries"), by HIP events on one stream: a batch of
2^20 rays through mrt_cast_rays_device on C2 (scene 5) and C4 (scene 8) -- pixel-centre camera rays
(a 1024 x 1024 grid under the scene's camera, row-major, so a wave's rays are neighbours) and
fixture-style random interior rays (seeded origins inside the scene's bounds, non-unit directions, a
third flagged inside; a wave's rays share nothing) -- with the 16-spp aux kernel of the same scene at
1024 x 1024 beside them as the yardstick (2^24 first hits).  Prints one line per figure: the median
and the minimum of `--rounds` rounds of `--reps` calls each, after a warm-up, and the rate.

    python tools/cast_cost.py [--rounds 7] [--reps 10]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import miniraytracer_amd as m  # noqa: E402
from aux_cost import timed  # noqa: E402

N = 1 << 20
NODE = np.dtype([("kind", "<u4"), ("a", "<u4"), ("b", "<u4"), ("mat", "<u4"), ("f", "<f4", (12,))])  # mrt_node
K_XY, K_XZ, K_YZ = 7, 8, 9


def room_bounds(view):
    """The box the view's axis-aligned rects span (both scenes are rooms): where the interior rays start."""
    import ctypes as C
    nodes = np.frombuffer((C.c_uint8 * (view.n_nodes * NODE.itemsize)).from_address(view.nodes), dtype=NODE)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for kind, (a, b, c) in ((K_XY, (0, 1, 2)), (K_XZ, (0, 2, 1)), (K_YZ, (1, 2, 0))):
        for f in nodes[(nodes["kind"] & 0xFF) == kind]["f"].astype(np.float64):
            for axis, v0, v1 in ((a, f[0], f[1]), (b, f[2], f[3]), (c, f[4], f[4])):
                lo[axis], hi[axis] = min(lo[axis], v0), max(hi[axis], v1)
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    return lo, hi


def camera_rays(cam, side=1024):
    """mrt_camera_pixel_ray's arithmetic for every pixel of a side x side image, in numpy float32."""
    f = np.float32
    c = {k: np.array(getattr(cam, k)[:3], dtype=f) for k in ("origin", "llcorner", "horz", "vert")}
    ys, xs = np.divmod(np.arange(side * side), side)
    s = ((xs.astype(f) + f(0.5)) / f(side))[:, None]
    t = ((ys.astype(f) + f(0.5)) / f(side))[:, None]
    rays = np.zeros(side * side, dtype=m.RAY_DTYPE)
    rays["o"] = c["origin"]
    rays["d"] = ((c["llcorner"] + s * c["horz"]) + t * c["vert"]) - c["origin"]
    rays["time"], rays["tmax"] = cam.time0, np.inf
    return rays


def interior_rays(lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo), np.asarray(hi)
    rays = np.zeros(n, dtype=m.RAY_DTYPE)
    rays["o"] = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    rays["d"] = (rng.uniform(-1, 1, (n, 3)) * rng.uniform(0.05, 20.0, (n, 1))).astype(np.float32)
    rays["time"] = rng.random(n).astype(np.float32)
    rays["tmax"] = np.inf
    rays["inside"] = rng.integers(0, 3, n) == 0
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    st = torch.cuda.Stream()
    sp = st.cuda_stream

    def line(what, t, n_hits):
        print(f"{what}: {t[0]:.4f} ms median, {t[1]:.4f} ms min ({t[2]} rounds x {t[3]} calls), {n_hits / t[0] * 1e-3:.0f} Mrays/s", flush=True)

    for cfg, sid in (("C2", 5), ("C4", 8)):
        sc = m.select_scene(sid, 1.0)
        r = m.Renderer(sc, 0)
        d_hits = torch.zeros(N * 32, dtype=torch.uint8, device="cuda")
        for what, rays in (("camera rays", camera_rays(sc.view.camera)), ("random interior rays", interior_rays(*room_bounds(sc.view), N, sid))):
            d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
            t = timed(torch, st, lambda: r.cast_rays_device(d_rays.data_ptr(), N, d_hits.data_ptr(), stream_ptr=sp), a.rounds, a.reps)
            hits = d_hits.cpu().numpy().view(m.HIT_DTYPE)
            line(f"{cfg} cast 2^20 {what} ({int((hits['mat'] != m.NO_HIT).sum())} hit)", t, N)
        d = m.render_desc(1024, 1024, 16)
        n = len(m.local_pixels(d))
        nrm, alb = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        r.prepare(d)
        line(f"{cfg} 1024x1024 aux kernel 16 spp", timed(torch, st, lambda: r.render_aux_device(d, nrm.data_ptr(), alb.data_ptr(), sp), a.rounds, max(2, a.reps // 3)),
             n * 16)
        r.close()


if __name__ == "__main__":
    main()
