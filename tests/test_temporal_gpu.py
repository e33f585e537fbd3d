"""Camera control and temporal reprojection on the MI355X: mrt_reproject_kernel bit for bit the host
mrt_reproject, mrt_scene_set_camera_device in stream order against the CPU backend under the same
camera, the whole orbit pipeline on the device, and both new device entries under graph capture."""
import numpy as np
import pytest

from test_aux_host import bits, ref_scene
from test_temporal_host import (F32, camera_f64, orbit_camera, pixel_dirs, plane_camera, second_camera, splitmix64, synth, with_camera)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(mrt):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    assert mrt.device_count() >= 1
    return mrt


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def device_reproject(gpu, c, nrm, alb, cam, hist=None, pn=None, pa=None, pcam=None, params=None):
    """reproject_device on a side stream; also checks that no input frame was written."""
    import torch
    h, w = c.shape[:2]
    host = [a for a in (c, nrm, alb, hist, pn, pa) if a is not None]
    t = [dev(a) for a in host]
    out = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    prev = [x.data_ptr() for x in t[3:]] if hist is not None else [0, 0, 0]
    gpu.reproject_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), cam, w, h, out.data_ptr(), *prev, prev_cam=pcam, params=params,
                         stream_ptr=st.cuda_stream)
    st.synchronize()
    for a, b in zip(t, host):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b))
    return out.cpu().numpy()


SHAPES = [(37, 23), (1, 1), (67, 45), (130, 5)]


# ---------------------------------------------------------------- 5. the kernel against the host
@pytest.mark.parametrize("w,h", SHAPES)
def test_device_reprojection_equals_host_on_random_guides(gpu, w, h):
    """Random guides (a fifth of the normals zero, some partial coverage) under two unrelated
    cameras; none of the shapes is a multiple of the 64 x 4 workgroup."""
    rng = np.random.default_rng(w * 1000 + h)
    c, hist, nrm, alb = synth(rng, w, h)
    _, _, pn, pa = synth(rng, w, h)
    for n in (nrm, pn):
        n[rng.random((h, w)) < 0.2, :3] = 0
        n[rng.random((h, w)) < 0.1, 3] = 0.75
    hist[..., 3] = rng.integers(1, 40, size=(h, w)).astype(F32)
    cam = gpu.make_camera(pos=(3, 2, 9), lookat=(0, 0, 0), vfov_deg=35, aspect=w / h, aperture=0.2, focus_dist=9)
    pcam = gpu.make_camera(pos=(-2, 4, 8), lookat=(1, 0, -1), vfov_deg=60, aspect=w / h, focus_dist=5)
    want = gpu.reproject(c, nrm, alb, cam, hist, pn, pa, pcam)
    assert np.array_equal(bits(device_reproject(gpu, c, nrm, alb, cam, hist, pn, pa, pcam)), bits(want))
    first = gpu.reproject(c, nrm, alb, cam)
    assert np.array_equal(bits(device_reproject(gpu, c, nrm, alb, cam)), bits(first)) and (first[..., 3] == 1).all()


@pytest.mark.parametrize("w,h", SHAPES)
def test_device_reprojection_equals_host_where_taps_blend(gpu, w, h):
    """A plane seen from two cameras a fraction of a pixel and a small turn apart, noisy normals and
    albedo around the tolerances: most pixels blend two to four taps, some lose one."""
    rng = np.random.default_rng(w * 1000 + h + 1)
    c, hist, _, _ = synth(rng, w, h)
    hist[..., 3] = rng.integers(1, 40, size=(h, w)).astype(F32)
    vfov = float(np.degrees(2 * np.arctan(0.2 / max(w / h, 1.0))))  # a narrow view either way: the plane's depth is nearly flat
    pcam = gpu.make_camera(pos=(0, 0, 0), lookat=(0, 0, -1), vfov_deg=vfov, aspect=w / h, focus_dist=1)
    pc = camera_f64(pcam)
    sx, sy = 0.37 * pc["horz"][0] / w * 4.0, -0.21 * pc["vert"][1] / h * 4.0
    cam = gpu.make_camera(pos=(sx, sy, 0), lookat=(sx + 0.002, sy - 0.001, -1), vfov_deg=vfov, aspect=w / h, focus_dist=1)
    guides = []
    for k in (cam, pcam):
        n = np.zeros((h, w, 4), dtype=F32)
        n[..., :3] = np.array([0, 0, 1]) + rng.normal(scale=0.2, size=(h, w, 3))
        n[..., 3] = 1
        a = np.zeros((h, w, 4), dtype=F32)
        a[..., :3] = 0.5 + rng.normal(scale=0.04, size=(h, w, 3))
        a[..., 3] = (4.0 / -pixel_dirs(k, w, h)[..., 2]) * (1 + rng.normal(scale=0.008, size=(h, w)))
        guides += [n, a]
    nrm, alb, pn, pa = guides
    p = gpu.default_temporal_params(depth_tol=0.05 if w > 1 else 0.5)
    want = gpu.reproject(c, nrm, alb, cam, hist, pn, pa, pcam, p)
    if w > 1:
        assert (want[..., 3] > 1).mean() > 0.5 and (want[..., 3] == 1).any()  # both ends of step 5 are compared
    assert np.array_equal(bits(device_reproject(gpu, c, nrm, alb, cam, hist, pn, pa, pcam, p)), bits(want))


# ---------------------------------------------------------------- 6. the camera in stream order
def frame(px, local, w, h):
    img = np.zeros((w * h, 4), dtype=np.float32)
    img[px] = local
    return img.reshape(h, w, 4)


class DeviceFrames:
    """One renderer's device buffers for a desc: colour, ray count, normal, albedo."""

    def __init__(self, gpu, r, d):
        import torch
        self.gpu, self.r, self.d = gpu, r, d
        self.px = gpu.local_pixels(d)
        r.prepare(d)
        self.out, self.nrm, self.alb = (torch.zeros((len(self.px), 4), dtype=torch.float32, device="cuda") for _ in range(3))
        self.rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.st = torch.cuda.Stream()
        torch.cuda.synchronize()

    def run(self, cam, d=None):
        """set_camera_device, render_device, render_aux_device on one stream; host copies."""
        d = d if d is not None else self.d
        for t in (self.out, self.nrm, self.alb, self.rays):
            t.zero_()
        import torch
        torch.cuda.synchronize()
        s = self.st.cuda_stream
        self.r.set_camera(cam, stream_ptr=s)
        self.r.render_device(d, self.out.data_ptr(), self.rays.data_ptr(), s)
        self.r.render_aux_device(d, self.nrm.data_ptr(), self.alb.data_ptr(), s)
        self.st.synchronize()
        w, h = d.width, d.height
        return [frame(self.px, t.cpu().numpy(), w, h) for t in (self.out, self.nrm, self.alb)], int(self.rays.item())


def cpu_frames(mrt, sc, cam, d):
    r = mrt.Renderer(sc, "cpu")
    r.set_camera(cam)
    img, rays = r.render(d)
    nrm, alb = r.render_aux(d)
    r.close()
    return [img, nrm, alb], rays


def same(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


@pytest.mark.parametrize("sid", [0, 5, 8])
def test_set_camera_device_equals_cpu_backend_under_that_camera(gpu, sid):
    """Scene 0 has a lens, motion blur and the sky; 5 the Cornell walk; 8 the triangle mesh."""
    sc = ref_scene(gpu, sid)
    cam_a, cam_b = sc.view.camera, second_camera(gpu, sc)
    d = gpu.render_desc(32, 32, 16)
    want_a, want_b = cpu_frames(gpu, sc, cam_a, d), cpu_frames(gpu, sc, cam_b, d)
    assert not same(want_a[0], want_b[0])
    r = gpu.Renderer(sc, 0)
    f = DeviceFrames(gpu, r, d)
    for cam, want in ((cam_b, want_b), (cam_a, want_a), (cam_b, want_b)):
        got, rays = f.run(cam)
        assert rays == want[1] and same(got, want[0])
    # the blocking form: mrt_render and mrt_render_aux follow it too
    for cam, want in ((cam_a, want_a), (cam_b, want_b)):
        r.set_camera(cam)
        img, rays = r.render(d)
        assert rays == want[1] and same([img] + list(r.render_aux(d)), want[0])
    r.close()


def test_set_camera_device_under_the_tolerance_contract(gpu):
    sc = ref_scene(gpu, 5)
    cam_a, cam_b = sc.view.camera, second_camera(gpu, sc)
    d = gpu.render_desc(32, 32, 16, numerics="fast")
    want = {}
    for name, cam in (("a", cam_a), ("b", cam_b)):
        ru = gpu.Renderer(with_camera(sc, cam), 0)  # uploaded with the camera in its view
        want[name] = ru.render(d)
        ru.close()
    assert not np.array_equal(bits(want["a"][0]), bits(want["b"][0]))
    r = gpu.Renderer(sc, 0)
    f = DeviceFrames(gpu, r, d)
    for name, cam in (("b", cam_b), ("a", cam_a)):
        got, rays = f.run(cam)
        assert rays == want[name][1] and np.array_equal(bits(got[0]), bits(want[name][0]))
    r.close()


# ---------------------------------------------------------------- 7. the pipeline on the device
def test_orbit_pipeline_on_the_device_equals_the_host_pipeline(gpu):
    """Three orbit frames at 64 x 64 on scene 5, exact contract, a row-major pixel list (so the
    local-pixel order is the frame's): set camera, render, feature buffers, reproject, all enqueued on
    one stream with no host work in between; the history frame equals the CPU backend's host
    pipeline bit for bit."""
    import torch
    w = h = 64
    frames, deg = 3, 2.0
    sc = ref_scene(gpu, 5)
    cams = [orbit_camera(gpu, sc, k, deg) for k in range(frames)]
    descs = [gpu.render_desc(w, h, 16, seed=splitmix64(gpu.MAIN_SEED + k), pixels=np.arange(w * h, dtype=np.uint32)) for k in range(frames)]
    rc = gpu.Renderer(sc, "cpu")
    want, prev = None, None
    for cam, d in zip(cams, descs):
        rc.set_camera(cam)
        img, _ = rc.render(d)
        nrm, alb = rc.render_aux(d)
        want = gpu.reproject(img, nrm, alb, cam) if want is None else gpu.reproject(img, nrm, alb, cam, want, prev[1], prev[2], prev[0])
        prev = (cam, nrm, alb)
    rc.close()
    assert (want[..., 3] == frames).mean() > 0.5

    r = gpu.Renderer(sc, 0)
    r.prepare(descs[0])
    buf = [[torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(4)] for _ in range(2)]  # colour, normal, albedo, history; two sets in turn
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = st.cuda_stream
    for k, (cam, d) in enumerate(zip(cams, descs)):
        c, n, a, hist = (t.data_ptr() for t in buf[k & 1])
        _, pn, pa, ph = (t.data_ptr() for t in buf[(k & 1) ^ 1])
        r.set_camera(cam, stream_ptr=s)
        r.render_device(d, c, rays.data_ptr(), s)
        r.render_aux_device(d, n, a, s)
        if k == 0:
            gpu.reproject_device(c, n, a, cam, w, h, hist, stream_ptr=s)
        else:
            gpu.reproject_device(c, n, a, cam, w, h, hist, ph, pn, pa, prev_cam=cams[k - 1], stream_ptr=s)
    st.synchronize()
    got = buf[(frames - 1) & 1][3].cpu().numpy()
    r.close()
    assert np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------- 8. graph capture
def test_graph_capture_of_aux_plus_reproject_and_of_set_camera(gpu):
    import torch
    w = h = 64
    sc = ref_scene(gpu, 5)
    cam0, cam1 = orbit_camera(gpu, sc, 0, 2.0), orbit_camera(gpu, sc, 1, 2.0)
    d = gpu.render_desc(w, h, 16, pixels=np.arange(w * h, dtype=np.uint32))
    rc = gpu.Renderer(sc, "cpu")
    rc.set_camera(cam0)
    img0, _ = rc.render(d)
    nrm0, alb0 = rc.render_aux(d)
    hist0 = gpu.reproject(img0, nrm0, alb0, cam0)
    rc.set_camera(cam1)
    img1, rays1 = rc.render(d)
    nrm1, alb1 = rc.render_aux(d)
    want = gpu.reproject(img1, nrm1, alb1, cam1, hist0, nrm0, alb0, cam0)
    rc.close()

    r = gpu.Renderer(sc, 0)
    r.prepare(d)
    rgb, ph, pn, pa = dev(img1), dev(hist0), dev(nrm0), dev(alb0)
    nrm, alb, out = (torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3))

    def enqueue(s):
        r.render_aux_device(d, nrm.data_ptr(), alb.data_ptr(), s)
        gpu.reproject_device(rgb.data_ptr(), nrm.data_ptr(), alb.data_ptr(), cam1, w, h, out.data_ptr(), ph.data_ptr(), pn.data_ptr(), pa.data_ptr(),
                             prev_cam=cam0, stream_ptr=s)

    r.set_camera(cam1)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    enqueue(side.cuda_stream)  # once outside the capture
    side.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        for b in (nrm, alb, out):
            b.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(nrm.cpu().numpy()), bits(nrm1)) and np.array_equal(bits(alb.cpu().numpy()), bits(alb1))
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    del graph

    # the camera store in a graph of its own: the capture itself stores nothing, the replay does
    r.set_camera(cam0)
    setcam = torch.cuda.CUDAGraph()
    with torch.cuda.graph(setcam):
        r.set_camera(cam1, stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    colour = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")

    def render():
        rays.zero_()
        r.render_device(d, colour.data_ptr(), rays.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return colour.cpu().numpy()

    assert np.array_equal(bits(render()), bits(img0))  # still camera 0: nothing ran during the capture
    setcam.replay()
    assert np.array_equal(bits(render()), bits(img1)) and int(rays.item()) == rays1
    del setcam
    r.close()
