"""The C restatement (oracle/mrt_oracle.c) and the host scene builder, pinned against the
reference's own code through the committed fixtures (tests/golden/, made by tools/make_golden.py
from oracle/_ref/mrt_ref_exact).  CPU only."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, SCENE_SIZES, canon_scene, golden_scene, golden_stream


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_pcg_kat_matches_reference(orc):
    kats = json.load(open(os.path.join(GOLDEN, "kat_pcg.json")))
    assert [hex(x) for x in kats[0]["rand32"][:6]] == ["0xa15c02b7", "0x7b47f409", "0xba1d3330", "0x83d2f293",
                                                       "0xbfa4784b", "0xcbed606e"]  # canonical pcg32 (42, 54)
    for k in kats:
        n = len(k["rand32"])
        assert orc.pcg_stream(k["state"], k["seq"], n).tolist() == k["rand32"]
        randf = orc.samplers(k["state"], k["seq"], n, 0)[:, 0]
        assert np.array_equal(randf.view(np.uint32), np.array(k["randf"], dtype=np.uint32))


@pytest.mark.parametrize("which,name", [(1, "in_sphere"), (2, "in_disk"), (3, "cosine_dir"), (4, "on_sphere")])
def test_sampler_kat_matches_reference(orc, which, name):
    for k in json.load(open(os.path.join(GOLDEN, "kat_pcg.json"))):
        got = orc.samplers(k["state"], k["seq"], len(k[name]), which)
        assert np.array_equal(got.view(np.uint32), np.array(k[name], dtype=np.uint32)), name


@pytest.mark.parametrize("sid", sorted(SCENE_SIZES))
def test_scene_builder_matches_reference(mrt, sid):
    """select_scene: camera, every primitive parameter, materials, textures (earthmap texel hash),
    object_list boxes, bvh_node / pod_bvh topology and node_order -- bit-exact."""
    w, h = SCENE_SIZES[sid]
    mine = canon_scene(mrt.select_scene(sid, w / h).dump_json())
    assert mine == golden_scene(sid)


@pytest.mark.parametrize("sid", sorted(SCENE_SIZES))
def test_oracle_hits_match_reference(mrt, orc, sid):
    w, h = SCENE_SIZES[sid]
    sc = mrt.select_scene(sid, w / h)
    rec = np.load(os.path.join(GOLDEN, f"hits_{sid}.npz"))["rays"]
    mism = 0
    for i, r in enumerate(rec):
        inside = int(r[7:8].view(np.int32)[0])
        hit = int(r[8:9].view(np.int32)[0])
        got, out = orc.hit(sc, r[0:3], r[3:6], r[6], inside, seed=i)
        if got != bool(hit) or (hit and not np.array_equal(out.view(np.uint32), r[9:16].view(np.uint32))):
            mism += 1
    assert mism == 0


STREAMS = [f"stream_{s}.npz" for s in range(10)] + ["stream_5_mode1.npz"]


@pytest.mark.parametrize("name", STREAMS)
def test_oracle_stream_render_matches_reference(mrt, orc, name):
    """Stream-matched render: every path's radiance and ray count, the draw()/draw2() image and the
    total ray count equal the reference's own trace() bit for bit."""
    g = golden_stream(name)
    sc = mrt.select_scene(g["sid"], g["w"] / g["h"])
    d = orc.desc(g["w"], g["h"], g["spp"], depth=g["depth"], mode=g["mode"], threads=8)
    img, rays, prgb, prays = orc.render(sc, d, paths=True)
    assert rays == g["rays"]
    assert np.array_equal(prays, g["path_rays"].astype(np.uint32))
    assert np.array_equal(prgb.view(np.uint32), g["path_rgb"].view(np.uint32))
    assert np.array_equal(img[..., :3].view(np.uint32), g["image"].view(np.uint32))


def test_shipped_reference_statistical_parity(mrt, orc):
    """The shipped (multithreaded, FMA-contracted, glibc libm) reference render of the Cornell box
    differs from the stream-matched restatement only by Monte-Carlo noise: same mean radiance
    within 3 sigma of the per-pixel noise, and comparable ray count."""
    g = np.load(os.path.join(GOLDEN, "shipped_5.npz"))
    ref = g["image"]
    sc = mrt.select_scene(5, 1.0)
    img, rays, _, _ = orc.render(sc, orc.desc(64, 64, 256, threads=8))
    mine = img[..., :3]
    diff = mine - ref
    # noise floor of two independent 256-spp renders at this size (measured in tools/make_golden.py run)
    rmse = float(np.sqrt((diff ** 2).mean()))
    assert rmse < 0.05, rmse
    assert abs(float(mine.mean() - ref.mean())) < 3e-3
    assert abs(rays / float(g["rays"][0]) - 1) < 0.005


@pytest.mark.parametrize("sid", [5, 8, 9, 7])
def test_restatement_within_tolerance_of_shipped_numerics(mrt, orc, sid):
    """North-star tolerance (per-pixel RMSE < 1e-3 vs the CPU image) against the reference AS SHIPPED
    -- FMA contraction, glibc libm -- on the same per-path streams (shipped_stream_<sid>_small.npz:
    Cornell, bunny, teapot-in-Cornell 128x128x256; book2 64x64x4096).  The exact build differs from
    it only by float rounding that occasionally sends a path another way.  Measured RMSE: 7.2e-4,
    2.9e-4, 4.1e-5, 7.7e-4 (3.8e-4 at full C2); ray totals within 2e-4 (book2: volume RNG)."""
    g = np.load(os.path.join(GOLDEN, f"shipped_stream_{sid}_small.npz"))
    _, w, h, spp, depth = (int(x) for x in g["meta"])
    sc = mrt.select_scene(sid, w / h)
    img, rays, _, _ = orc.render(sc, orc.desc(w, h, spp, depth=depth, threads=8))
    d = img[..., :3].astype(np.float64) - g["image"]
    assert float(np.sqrt((d ** 2).mean())) < 1e-3
    assert np.abs(d.reshape(-1, 3).mean(axis=0)).max() < 1e-4
    assert abs(rays / float(g["rays"][0]) - 1) < 1e-3


def test_worker_seeds_match_reference_main(mrt):
    """main.cpp:357-361: the (initstate, initseq) main() draws for its workers after select_scene.
    Scene 5 consumes no RNG while it is built, so these are the SURVEY 8(c) vector (clang's left-to-
    right evaluation of `(uint64(rand32()) << 32) | rand32()`)."""
    sc = mrt.select_scene(5, 1.0)
    assert sc.worker_seeds(2) == [(6838637184523169570, 909894286423444019), (11866281134630579356, 5863659702987752277)]


REFSEQ = [(s, md) for s in (0, 5, 7, 8) for md in (0, 1)]


@pytest.mark.parametrize("sid,mode", REFSEQ)
def test_oracle_reproduces_reference_threads1_mode(mrt, orc, sid, mode):
    """The reference's OWN deterministic mode (-threads 1 -mode 0/1, fixtures refseq_<sid>_m<mode>
    from the exact reference build): one worker PCG stream seeded as main() seeds it, tiles in
    work_queue order, pixels row by row, samples (mode 0) or sample-major passes (mode 1).  The C
    restatement's reference-RNG-order mode reproduces G_linearBackBuffer and G_rayCounter bit for
    bit."""
    g = np.load(os.path.join(GOLDEN, f"refseq_{sid}_m{mode}.npz"))
    _, w, h, spp, depth, ts, md, rays = (int(x) for x in g["meta"])
    assert md == mode
    sc = mrt.select_scene(sid, w / h)
    img, r = orc.render_ref_order(sc, orc.desc(w, h, spp, depth=depth, mode=mode), tile_size=ts)
    assert r == rays
    assert np.array_equal(img[..., :3].view(np.uint32), g["image"].view(np.uint32))


def test_oracle_pdfs_match_reference(mrt, orc):
    """The restatement's object pdfs (obj_pdf_value / obj_pdf_generate: sphere, moving sphere,
    xz_rect, the default of scene_object.h:24-29 for an xy_rect, object_lists of two and three)
    against the reference's own classes (tests/golden/kat_pdf.npz, harness --h-mode pdf): pdf_value
    bits for seeded (origin, dir, time) rows -- origins inside the sphere and directions that miss
    included -- and pdf_generate's vector plus the stream's next rand32, which pins the draw count.
    No reference scene exercises these paths; the synthetic catalogue relies on them."""
    import synth_scenes as ss
    g = np.load(os.path.join(GOLDEN, "kat_pdf.npz"))
    s = ss.Synth(mrt.select_scene(5, 1.0)).clear()
    mat = s.lambertian(0.5, 0.5, 0.5)
    prim = []
    for p in g["prims"]:
        kind, f = int(p[0]), p[1:]
        if kind == ss.K_SPHERE:
            moving = f[7] - f[6] > np.finfo(np.float32).eps  # sphere.h:21
            prim.append(s.node(kind, mat=mat, f=f, flags=ss.F_MOVING if moving else 0))
        else:
            prim.append(s.node(kind, mat=mat, f=f[:6]))
    objs = prim + [s.list([prim[i] for i in g["list2"]]), s.list([prim[i] for i in g["list3"]])]
    s.root = objs[-1]
    rows, n = g["rows"], len(g["rows"])
    state0, seq = (int(x) for x in g["stream"])
    states = np.arange(n, dtype=np.uint64) + np.uint64(state0)
    assert (np.linalg.norm(rows[::4, :3] - g["prims"][0][1:4], axis=1) < g["prims"][0][9]).all()  # origins inside the sphere
    for k, node in enumerate(objs):
        value, gen, nxt = orc.pdf(s, node, rows, states, seq)
        want = g["value"][:, k]
        if k == 3:  # the xy_rect has no pdf of its own
            assert (want == 0).all()
        else:  # the rows hold hits and misses of every other object
            assert (want == 0).any() and (want != 0).any(), k
        assert np.array_equal(value.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), f"pdf_value of object {k}"
        assert np.array_equal(gen.view(np.uint32), np.ascontiguousarray(g["gen"][:, k]).view(np.uint32)), f"pdf_generate of object {k}"
        assert np.array_equal(nxt, g["next"][:, k]), f"draw count of object {k}"
