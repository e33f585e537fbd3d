"""Device cost of temporal reprojection (DESIGN.md "Camera and temporal accumulation"), on C2 (scene
5, 500 x 500, tolerance contract, the bench's): mrt_reproject_kernel on the frames of a 2-degree
orbit step beside what else a frame of a sequence costs -- the 16-spp render, the feature buffers,
one a-trous pass, the camera store -- by HIP events on one stream.  Prints one line per figure: the
median and the minimum of the rounds, after a warm-up; then the share of the pixels that kept history.

    python tools/temporal_cost.py [--rounds 7] [--reps 10]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def orbit_camera(scene, k, deg, centre=(278.0, 278.0, 278.0)):
    p = scene.camera_params()
    a = np.radians(k * deg)
    dx, dz = p.pos[0] - centre[0], p.pos[2] - centre[2]
    return m.make_camera(p, pos=(centre[0] + dx * np.cos(a) + dz * np.sin(a), p.pos[1], centre[2] - dx * np.sin(a) + dz * np.cos(a)), lookat=centre)


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
    sc = m.select_scene(5, 1.0)
    r = m.Renderer(sc, 0)
    cams = [orbit_camera(sc, k, 2.0) for k in range(2)]
    px = np.arange(w * h, dtype=np.uint32)  # row-major: the local-pixel order is the frame's
    d = m.render_desc(w, h, 16, numerics="fast", pixels=px)
    r.prepare(d)
    fr = [[torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(2)]  # colour, normal, albedo per frame
    hist = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    tmp = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    with torch.cuda.stream(st):
        for k in range(2):
            r.set_camera(cams[k], stream_ptr=sp)
            r.render_device(d, fr[k][0].data_ptr(), rays.data_ptr(), sp)
            r.render_aux_device(d, fr[k][1].data_ptr(), fr[k][2].data_ptr(), sp)
        m.reproject_device(fr[0][0].data_ptr(), fr[0][1].data_ptr(), fr[0][2].data_ptr(), cams[0], w, h, hist[0].data_ptr(), stream_ptr=sp)
        st.synchronize()
    c, n, al = (t.data_ptr() for t in fr[1])
    # the render and the feature buffers in the tile layout (the bench's; a pixel list is checked on the host at every call)
    dt = m.render_desc(w, h, 16, numerics="fast")
    r.prepare(dt)
    loc = [torch.zeros((h * w, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
    line("C2 500x500 render 16 spp (fast), enqueued", timed(torch, st, lambda: r.render_device(dt, loc[0].data_ptr(), rays.data_ptr(), sp), a.rounds, a.reps))
    line("C2 500x500 feature buffers 16 spp", timed(torch, st, lambda: r.render_aux_device(dt, loc[1].data_ptr(), loc[2].data_ptr(), sp), a.rounds, a.reps))
    p1 = m.default_denoise_params()
    p1.iterations = 1
    line("C2 500x500 one a-trous pass", timed(torch, st, lambda: m.denoise_device(c, n, al, w, h, hist[1].data_ptr(), tmp.data_ptr(), p1, sp), a.rounds, a.reps))
    line("C2 500x500 reprojection, 2 degree orbit step",
         timed(torch, st, lambda: m.reproject_device(c, n, al, cams[1], w, h, hist[1].data_ptr(), hist[0].data_ptr(), fr[0][1].data_ptr(),
                                                     fr[0][2].data_ptr(), prev_cam=cams[0], stream_ptr=sp), a.rounds, a.reps))
    line("C2 500x500 reprojection, still camera",
         timed(torch, st, lambda: m.reproject_device(c, n, al, cams[1], w, h, hist[1].data_ptr(), hist[0].data_ptr(), n, al, prev_cam=cams[1],
                                                     stream_ptr=sp), a.rounds, a.reps))
    line("C2 500x500 reprojection, first frame (no history)",
         timed(torch, st, lambda: m.reproject_device(c, n, al, cams[1], w, h, hist[1].data_ptr(), stream_ptr=sp), a.rounds, a.reps))
    line("camera store (mrt_scene_set_camera_device)", timed(torch, st, lambda: r.set_camera(cams[1], stream_ptr=sp), a.rounds, a.reps))
    m.reproject_device(c, n, al, cams[1], w, h, hist[1].data_ptr(), hist[0].data_ptr(), fr[0][1].data_ptr(), fr[0][2].data_ptr(), prev_cam=cams[0],
                       stream_ptr=sp)
    st.synchronize()
    out = hist[1].cpu().numpy()
    cov = fr[1][1].cpu().numpy()[..., 3]
    print(f"C2 500x500, 2 degree step, 16 spp (fast): history kept at {(out[..., 3] > 1).mean():.4f} of the pixels, fully covered {(cov == 1).mean():.4f}")
    r.close()


if __name__ == "__main__":
    main()
