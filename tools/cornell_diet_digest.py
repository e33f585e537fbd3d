#!/usr/bin/env python3
"""Digests of the Cornell kernels' per-path results on the cases that matter when the loop's skeleton
is trimmed: the diffuse scatter's normal and attenuation re-read by the hit's identity instead of
carried, lane masks kept as masks, the radiance pointer's load moved, and the refill's claim made in 32
bits on the scalar unit.  Every path keeps its operations, their order and its stream positions.

  walls, walls_dD     a material of its own on every wall and box face, the box's rotation negated
                      (tools/cornell_table_digest.py walls_scene); depth limits D = 1, 2: a scatter is
                      followed at once by the path's end
  sphere, sphere_dD   the sphere lambertian (identity 13, no table normal), 64x64x16; D = 1, 2
  offlight            another rect as the biased object: the pdf takes the leaf path
  paths_N             scene 5 with N = 1, 63, 64, 65, 129 paths at 1 spp
  rows_wW             scene 5, W x 1 pixels at 4 spp, W = 1, 2, 31, 33, 63, 64, 65
  pair                two renders in a row on ONE renderer, depth 32 then 2
  glass               the glass-heavy scene: all 64 lanes take the glass branch
  ragged_N            N = 8191, 8193 (8 k -+ 1), 8460 paths; 500 paths (below 64 per partition, as paths_129);
                      200 paths (below one claim)
  dyn_8k1, dyn_8km1   2099601 = 8 k + 1 and 6759999 = 8 k - 1 paths: more than every wave's static claim,
                      so the partitions' counters hand out claims; in the first all of them are small
                      (the whole launch is tail zone), in the second a partition's claims start at full
                      size and shrink at its tail zone's edge
  chunked             a render in launches of 4 samples (s0 > 0 from the second): the image's bits
  pixel_list          five listed pixels of a 24x24 image at 16 spp
  nosig_*             rows_w33, ragged_8460 and chunked through the interpreter's queue kernel (MRT_NO_SIG=1)

tools/fast_path_digest.py's method: numerics="fast", MRT_RF_PATH_DEBUG (the per-path ray count is
stored beside the radiance), sha256 of the per-path radiance bits and ray counts.
tests/test_cornell_diet.py compares with the committed tests/golden/cornell_diet_parent.json, this
tool's output with the PARENT commit's library (never regenerated from the tree under test).
  python tools/cornell_diet_digest.py [out.json]      (default: stdout)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cornell_resident_digest as crd  # noqa: E402
import cornell_start_digest as csd  # noqa: E402
import fast_path_digest as fpd  # noqa: E402

V_INTERP = csd.V_INTERP
PIXEL_LIST = (3, 100, 101, 300, 575)  # row-major indices of a 24x24 image

_PATHS = {1: (1, 1), 63: (9, 7), 64: (8, 8), 65: (13, 5), 129: (43, 3)}
_RAGGED = {8191: (8191, 1), 8193: (2731, 3), 500: (25, 20), 200: (20, 10)}
# (name, scene, width, height, spp, depth limits of the renders in order, chunk_samples or 0,
#  MRT_NO_SIG, pixel list or None)
_ROW33 = ("rows_w33", 5, 33, 1, 4, (32,), 0)
_R8460 = ("ragged_8460", 5, 45, 47, 4, (32,), 0)
_CHUNKED = ("chunked", 5, 24, 24, 16, (32,), 4)
CASES = [("walls", "walls", 24, 24, 4, (32,), 0, False, None),
         ("walls_d1", "walls", 16, 16, 4, (1,), 0, False, None),
         ("walls_d2", "walls", 16, 16, 4, (2,), 0, False, None),
         ("sphere", "lambsphere", 64, 64, 16, (32,), 0, False, None),
         ("sphere_d1", "lambsphere", 16, 16, 4, (1,), 0, False, None),
         ("sphere_d2", "lambsphere", 16, 16, 4, (2,), 0, False, None),
         ("offlight", "offlight", 24, 24, 4, (32,), 0, False, None)] + [
    (f"paths_{n}", 5, wh[0], wh[1], 1, (32,), 0, False, None) for n, wh in _PATHS.items()] + [
    (f"rows_w{w}", 5, w, 1, 4, (32,), 0, False, None) for w in (1, 2, 31, 63, 64, 65)] + [_ROW33 + (False, None)] + [
    ("pair", 5, 13, 5, 1, (32, 2), 0, False, None),
    ("glass", "glass", 16, 16, 4, (32,), 0, False, None)] + [
    (f"ragged_{n}", 5, wh[0], wh[1], 1, (32,), 0, False, None) for n, wh in _RAGGED.items()] + [
    _R8460 + (False, None),
    ("dyn_8k1", 5, 1449, 1449, 1, (32,), 0, False, None),
    ("dyn_8km1", 5, 2601, 2599, 1, (32,), 0, False, None),
    _CHUNKED + (False, None),
    ("pixel_list", 5, 24, 24, 16, (32,), 0, False, PIXEL_LIST)] + [
    ("nosig_" + c[0],) + c[1:] + (True, None) for c in (_ROW33, _R8460, _CHUNKED)]


def n_paths(case):
    return (len(case[8]) if case[8] else case[2] * case[3]) * case[4]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest_case(mrt, case):
    name, sid, w, h, spp, depths, chunk, nosig, pixels = case
    old = os.environ.get("MRT_NO_SIG")
    try:
        if nosig:
            os.environ["MRT_NO_SIG"] = "1"  # read at upload
        r = mrt.Renderer(crd.scene_of(mrt, sid, 1.0 if max(w, h) > 8 * min(w, h) else w / h), 0)
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
