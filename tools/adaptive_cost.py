"""Device cost of the sample moments and the adaptive render (DESIGN.md "Adaptive sampling"), on C2
(scene 5, 500 x 500, tolerance contract, the bench's): mrt_moments_kernel on a radiance chunk of the
render's shape at 16 and 1024 spp beside that render -- its whole enqueued time and its path kernel
(HIP events; the difference is the fold, the hand-over and the launch gaps) -- by HIP events on one
stream, and the blocking adaptive render (the library's defaults; a 16-spp base against blocking
uniform renders at 64 and 100 spp, a 64-spp base against 256 spp) in wall milliseconds and rays, in
interleaved rounds.  Prints one
line per figure: the median and the minimum of the rounds, after a warm-up.

    python tools/adaptive_cost.py [--rounds 7] [--reps 10]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import miniraytracer_amd as m  # noqa: E402


def timed(torch, stream, fn, rounds, reps):
    """ms per call: (median, min) over rounds; events on the stream the calls are enqueued on (as tools/aux_cost.py)."""
    with torch.cuda.stream(stream):
        for _ in range(2):
            fn()
        stream.synchronize()
        ms = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(reps):
                fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b) / reps)
    return float(np.median(ms)), float(min(ms)), rounds, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    st = torch.cuda.Stream()
    sp = st.cuda_stream

    def line(what, t):
        print(f"{what}: {t[0]:.4f} ms median, {t[1]:.4f} ms min ({t[2]} rounds x {t[3]} calls)", flush=True)

    w = h = 500
    r = m.Renderer(m.select_scene(5, 1.0), 0)
    loc = torch.zeros((h * w, 4), dtype=torch.float32, device="cuda")
    mom = torch.zeros((h * w, 4), dtype=torch.float32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    for spp, rounds, reps in ((16, a.rounds, a.reps), (1024, max(3, a.rounds // 2), 3)):
        d = m.render_desc(w, h, spp, numerics="fast")
        n = len(m.local_pixels(d))
        r.prepare(d)
        line(f"C2 500x500 render {spp} spp (fast), enqueued", timed(torch, st, lambda: r.render_device(d, loc.data_ptr(), rays.data_ptr(), sp), rounds, reps))
        ks = []
        for _ in range(rounds):  # the path kernel's own events (mrt_kernel_ms) of single renders
            r.render_device(d, loc.data_ptr(), rays.data_ptr(), sp)
            st.synchronize()
            ks.append(r.kernel_ms()[0])
        print(f"C2 500x500 path kernel {spp} spp (fast): {np.median(ks):.4f} ms median, {min(ks):.4f} ms min ({rounds} renders)", flush=True)
        # a chunk of the render's shape: [s][local pixel] float3 (values do not change the kernel's time)
        rad = torch.rand((spp, n, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        line(f"C2 500x500 moments kernel {spp} spp ({rad.numel() * 4 / 1e6:.0f} MB of radiance)",
             timed(torch, st, lambda: m.moments_device(rad.data_ptr(), n, spp, mom.data_ptr(), 0, sp), rounds, reps))
        del rad
    del loc, mom, rays
    torch.cuda.synchronize()

    # ---- the blocking entry points, interleaved: adaptive (the library's defaults) against uniform renders --
    # a 16-spp base against 64 and 100 spp, and a 64-spp base (passes at 256 and 1024 spp) against 256 spp
    p = m.default_adaptive_params()
    for base_spp, uniform in ((16, (64, 100)), (64, (256,))):
        base = m.render_desc(w, h, base_spp, numerics="fast")
        cases = [(f"adaptive {base_spp} spp base", lambda: r.render_adaptive(base, p)[1:])]
        for u in uniform:
            cases.append((f"uniform {u} spp", lambda u=u: (None, r.render(m.render_desc(w, h, u, numerics="fast"))[1])))
        ms = {k: [] for k, _ in cases}
        info = {}
        for rnd in range(a.rounds + 1):  # round 0 warms up
            for k, fn in cases:
                t0 = time.perf_counter()
                mo, nr = fn()
                dt = (time.perf_counter() - t0) * 1e3
                if rnd:
                    ms[k].append(dt)
                info[k] = (mo, nr)
        for k, _ in cases:
            mo, nr = info[k]
            extra = ""
            if mo is not None:
                spent = mo[..., 3]
                n1, n2 = base_spp, base_spp + 4 * base_spp
                extra = (f", max_passes {p.max_passes} atol {p.atol:g} rtol {p.rtol:g}: {spent.mean():.1f} spp mean, refined "
                         f"{int((spent > n1).sum())} then {int((spent > n2).sum())} of {spent.size} pixels")
            print(f"C2 500x500 {k} (fast, blocking call): {np.median(ms[k]):.3f} ms median, {min(ms[k]):.3f} ms min ({a.rounds} rounds), "
                  f"{nr} rays{extra}", flush=True)
    r.close()


if __name__ == "__main__":
    main()
