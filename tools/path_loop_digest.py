#!/usr/bin/env python3
"""Digests of the tolerance contract's per-path results for the path kernel's loops that the Cornell
digests (tools/fast_path_digest.py and the cornell_*_digest.py tools) do not reach: the resumable
room + mesh loop (scenes 8 and 9) and the plain loop (the bvh_node treelet kernels of scenes 0 and 7,
Cornell smoke, the generic machine, the mesh interpreter), each on 1, 65 and 2304 paths, and on 8460
(no multiple of 8 partitions x 256: dynamic claims and the tail zone run) where groups are large or
the loop yields.  One case renders without MRT_RF_PATH_DEBUG, so the retrace kernel and its LDS run.

tools/fast_path_digest.py's method: numerics="fast", MRT_RF_PATH_DEBUG, sha256 of the per-path
radiance bits and ray counts.  tests/test_path_loops.py compares with the committed
tests/golden/pathloops_parent.json, this tool's output with the PARENT commit's library (never
regenerated from the tree under test).
  python tools/path_loop_digest.py [out.json]      (default: stdout)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fast_path_digest as fpd  # noqa: E402

_SIZES = ((1, 1, 1), (13, 5, 1), (24, 24, 4))
_RAGGED = (45, 47, 4)
# (name, scene, width, height, spp, depth limits of the renders in order, upload hook or None)
CASES = [(f"s{s}_{w}x{h}x{n}", s, w, h, n, (32,), None) for s in (0, 6, 7, 8, 9) for w, h, n in _SIZES] + [
    (f"s{s}_ragged", s) + _RAGGED + ((32,), None) for s in (9, 7, 8)] + [
    (f"generic_s5_{w}x{h}x{n}", 5, w, h, n, (32,), "MRT_FORCE_GENERIC") for w, h, n in _SIZES[1:]] + [
    (f"nosig_s9_{w}x{h}x{n}", 9, w, h, n, (32,), "MRT_NO_SIG") for w, h, n in _SIZES[1:]] + [
    ("s9_pair", 9, 13, 5, 1, (32, 2), None)]
# the hand-over case (no debug flag): scene 5 at the smallest of these sizes at which the parent lists
# at least four paths for the exact arithmetic
RETRACE_SIZES = ((64, 64, 64), (128, 128, 64), (128, 128, 256))
RETRACE_MIN = 4


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _renderer(mrt, sid, aspect, hook):
    old = os.environ.get(hook) if hook else None
    try:
        if hook:
            os.environ[hook] = "1"  # read at upload
        return mrt.Renderer(mrt.select_scene(sid, aspect), 0)
    finally:
        if hook:
            if old is None:
                del os.environ[hook]
            else:
                os.environ[hook] = old


def digest_case(mrt, case):
    name, sid, w, h, spp, depths, hook = case
    r = _renderer(mrt, sid, w / h, hook)
    out = {"renders": []}
    for depth in depths:
        rgb, rays, total, _ = fpd.render_paths(mrt, r, w, h, spp, depth)
        assert int(rays.sum()) == total, (name, int(rays.sum()), total)
        out["renders"].append({"radiance_sha256": _sha(np.ascontiguousarray(rgb).view(np.uint32)), "rays_sha256": _sha(rays),
                               "depth": depth, "rays": int(total)})
    ki = r.kernel_info()
    out.update({"kernel_features": int(ki["kernel_features"]), "build": int(ki["build"])})
    r.close()
    return out


def digest_retrace(mrt, size):
    """Scene 5, tolerance contract, no debug flag: the image's bits, the ray total and the paths the
    fast kernel handed to the retrace kernel."""
    w, h, spp = size
    r = mrt.Renderer(mrt.select_scene(5, w / h), 0)
    img, total = r.render(mrt.render_desc(w, h, spp, numerics="fast"))
    ki = r.kernel_info()
    r.close()
    return {"size": list(size), "image_sha256": _sha(np.ascontiguousarray(img).view(np.uint32)), "rays": int(total),
            "handed_over": int(ki["handed_over"]), "kernel_features": int(ki["kernel_features"]), "build": int(ki["build"])}


def main():
    import miniraytracer_amd as mrt
    out = {c[0]: digest_case(mrt, c) for c in CASES}
    for size in RETRACE_SIZES:
        out["retrace"] = digest_retrace(mrt, size)
        if out["retrace"]["handed_over"] >= RETRACE_MIN:
            break
    text = json.dumps(out, indent=1, sort_keys=True) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
