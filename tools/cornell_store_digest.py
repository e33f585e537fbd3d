#!/usr/bin/env python3
"""Digests of the Cornell kernels' per-path results on the cases that matter to WHERE a finished path's
radiance is stored and to HOW a refill of the queue of path starts finds each start's (local pixel,
sample row): a store issued where the path ends (not held for an iteration) must write the same three
words at the same address, beside the ray count's store, for the last path of a launch as for every
other; path coordinates, in whatever form a refill takes them (each lane's own quotient, or a run's start
plus the lane offset), must be right for every row end inside a refill; and a start's time draw must
still move the stream where the kernel no longer makes its value.

  store_N_dD          scene 5 with N = 1, 63, 64, 65, 129 paths at 1 spp under depth limits D = 1, 32
                      (MRT_RF_PATH_DEBUG: the ray count's store sits beside the radiance store)
  store_pair          two renders in a row on ONE renderer, depth 32 then 1: each render's digests
  rows_wW             scene 5, W x 1 pixels at 16 spp, W = 1, 5, 63, 64, 65: sixteen, twelve and one
                      sample rows inside one refill; a row end before, at and after a wave's 64th start
                      (the scene's square camera on the one-row image, so the room fills the samples'
                      columns: a path started at another pixel's or sample's coordinates differs)
  pixel_list          five listed pixels of a 24x24 image at 16 spp
  chunked             one render in several launches (chunk_samples 4): the image's bits and the ray
                      total (MRT_RF_PATH_DEBUG keeps a render in one launch)
  ragged              45x47 at 4 spp: 8460 paths, no multiple of 8 partitions x 256
  lens_shutter        tools/cornell_start_digest.py's camera with a lens and a shutter: the time draw
                      reaches the ray, so the stream must still step over it
  nosig_*             rows_w5, rows_w65 and chunked through the interpreter's queue kernel (MRT_NO_SIG=1)

tools/fast_path_digest.py's method: numerics="fast", MRT_RF_PATH_DEBUG, sha256 of the per-path
radiance bits and ray counts.  tests/test_cornell_store.py compares with the committed
tests/golden/cornell_store_parent.json, this tool's output with the PARENT commit's library (never
regenerated from the tree under test).
  python tools/cornell_store_digest.py [out.json]      (default: stdout)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cornell_start_digest as csd  # noqa: E402
import fast_path_digest as fpd  # noqa: E402

V_INTERP = csd.V_INTERP
PIXEL_LIST = (3, 100, 101, 300, 575)  # row-major indices of a 24x24 image

_PATHS = {1: (1, 1), 63: (9, 7), 64: (8, 8), 65: (13, 5), 129: (43, 3)}
# (name, scene, width, height, spp, depth limits of the renders in order, chunk_samples or 0,
#  MRT_NO_SIG, pixel list or None)
_ROWS = [(f"rows_w{w}", 5, w, 1, 16, (32,), 0) for w in (1, 5, 63, 64, 65)]
_CHUNKED = ("chunked", 5, 24, 24, 16, (32,), 4)
CASES = [(f"store_{n}_d{d}", 5, wh[0], wh[1], 1, (d,), 0, False, None) for n, wh in _PATHS.items() for d in (1, 32)] + [
    ("store_pair", 5, 13, 5, 1, (32, 1), 0, False, None)] + [c + (False, None) for c in _ROWS] + [
    ("pixel_list", 5, 24, 24, 16, (32,), 0, False, PIXEL_LIST),
    _CHUNKED + (False, None),
    ("ragged", 5, 45, 47, 4, (32,), 0, False, None),
    ("lens_shutter", "lens", 32, 32, 9, (32,), 0, False, None)] + [
    ("nosig_" + c[0],) + c[1:] + (True, None) for c in (_ROWS[1], _ROWS[4], _CHUNKED)]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest_case(mrt, case):
    name, sid, w, h, spp, depths, chunk, nosig, pixels = case
    old = os.environ.get("MRT_NO_SIG")
    try:
        if nosig:
            os.environ["MRT_NO_SIG"] = "1"  # read at upload
        r = mrt.Renderer(csd.scene_of(mrt, sid, 1.0 if h == 1 else w / h), 0)
    finally:
        if nosig:
            if old is None:
                del os.environ["MRT_NO_SIG"]
            else:
                os.environ["MRT_NO_SIG"] = old
    out = {"renders": []}
    for depth in depths:
        if chunk:
            img, total = r.render(mrt.render_desc(w, h, spp, depth=depth, numerics="fast", chunk_samples=chunk))
            e = {"image_sha256": _sha(np.ascontiguousarray(img).view(np.uint32))}
        else:
            kw = {} if pixels is None else {"pixels": np.asarray(pixels, dtype=np.uint32)}
            rgb, rays, total, px = fpd.render_paths(mrt, r, w, h, spp, depth, **kw)
            assert int(rays.sum()) == total, (name, int(rays.sum()), total)
            assert pixels is None or sorted(int(p) for p in px) == sorted(pixels), (name, px)
            e = {"radiance_sha256": _sha(np.ascontiguousarray(rgb).view(np.uint32)), "rays_sha256": _sha(rays)}
        e.update({"depth": depth, "rays": int(total)})
        out["renders"].append(e)
    out["kernel_features"] = int(r.kernel_info()["kernel_features"])
    r.close()
    return out


def main():
    import miniraytracer_amd as mrt
    out = {c[0]: digest_case(mrt, c) for c in CASES}
    text = json.dumps(out, indent=1, sort_keys=True) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
