"""Device cost of the first-hit feature buffers and the a-trous filter (DESIGN.md "Feature buffers
and denoise"), by HIP events on one stream: on C2 (scene 5, 500 x 500) the aux kernel at 16 spp and
the filter's passes next to the 16-spp and the 1024-spp render (tolerance contract, the bench's),
and the aux kernel on C5 (scene 7, 2048 x 2048).  Prints one line per figure: the median and the
minimum of `--rounds` rounds of `--reps` calls each, after a warm-up.

    python tools/aux_cost.py [--rounds 7] [--reps 10] [--passes 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import miniraytracer_amd as m  # noqa: E402


def timed(torch, stream, fn, rounds, reps):
    """ms per call: (median, min) over rounds; events on the stream the calls are enqueued on."""
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
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    st = torch.cuda.Stream()
    sp = st.cuda_stream

    def line(what, t):
        print(f"{what}: {t[0]:.4f} ms median, {t[1]:.4f} ms min ({t[2]} rounds x {t[3]} calls)", flush=True)

    # ---- C2: scene 5, 500 x 500
    w = h = 500
    r = m.Renderer(m.select_scene(5, 1.0), 0)
    d16 = m.render_desc(w, h, 16, numerics="fast")
    d1024 = m.render_desc(w, h, 1024, numerics="fast")
    # the filter's input: the 16-spp frame and its buffers as whole row-major frames (host entry points)
    img, _ = r.render(d16)
    hn, ha = r.render_aux(d16)
    rgb, nrm, alb = (torch.from_numpy(x).cuda() for x in (img, hn, ha))
    out, tmp, loc, ln, la = (torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(5))
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    r.prepare(d16)
    line("C2 500x500 render 16 spp (fast)", timed(torch, st, lambda: r.render_device(d16, loc.data_ptr(), rays.data_ptr(), sp), a.rounds, a.reps))
    line("C2 500x500 aux kernel 16 spp", timed(torch, st, lambda: r.render_aux_device(d16, ln.data_ptr(), la.data_ptr(), sp), a.rounds, a.reps))
    for passes in sorted({1, 2, 3, a.passes}):
        p = m.default_denoise_params()
        p.iterations = passes
        line(f"C2 500x500 a-trous filter {passes} pass(es)",
             timed(torch, st, lambda: m.denoise_device(rgb.data_ptr(), nrm.data_ptr(), alb.data_ptr(), w, h, out.data_ptr(), tmp.data_ptr(), p, sp),
                   a.rounds, a.reps))
    r.prepare(d1024)
    line("C2 500x500 render 1024 spp (fast)",
         timed(torch, st, lambda: r.render_device(d1024, loc.data_ptr(), rays.data_ptr(), sp), max(3, a.rounds // 2), 3))
    r.close()
    del rgb, nrm, alb, out, tmp, loc, ln, la

    # ---- C5: scene 7, 2048 x 2048
    w = h = 2048
    r = m.Renderer(m.select_scene(7, 1.0), 0)
    d = m.render_desc(w, h, 16)
    n = len(m.local_pixels(d))
    nrm, alb = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    r.prepare(d)
    line("C5 2048x2048 aux kernel 16 spp", timed(torch, st, lambda: r.render_aux_device(d, nrm.data_ptr(), alb.data_ptr(), sp), a.rounds, max(2, a.reps // 3)))
    r.close()


if __name__ == "__main__":
    main()
