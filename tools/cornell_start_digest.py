#!/usr/bin/env python3
"""Digests of the Cornell kernels' per-path results on cases that tools/fast_path_digest.py and
tools/cornell_table_digest.py do not have: the cosine scatter's basis on a per-ray normal beside table
normals, a camera with a lens and a shutter, launches of a few paths, a render in several launches, and
the interpreter's queue kernel.  Work on the cosine scatter's basis or on how the wave's queue makes its
path starts must leave every path's operations, operands and stream order as they are.

  sphere_lambertian   scene 5 with the sphere's material made lambertian: identity 13 scatters by the
                      cosine pdf with a per-ray normal while the walls' normals are table constants
  lens_shutter        scene 5 with a lens radius > 0 and time0 != time1: the camera's disk point, the
                      path's (u, v) and its time draw all reach the ray
  paths_N             scene 5 with N = 1, 63, 64, 65, 129 paths at 1 spp: fewer paths than lanes, one
                      full refill, a refill with one path, two refills and a remainder
  chunked             one render in several launches (chunk_samples): the image's bits and the ray total
                      (MRT_RF_PATH_DEBUG keeps a render in one launch, so there are no per-path results)
  nosig_*             the last three again through the interpreter's queue kernel (MRT_NO_SIG=1 at upload)

tools/fast_path_digest.py's method: numerics="fast", MRT_RF_PATH_DEBUG, sha256 of the per-path
radiance bits and ray counts.  tests/test_cornell_starts.py compares with the committed
tests/golden/cornell_starts_parent.json, this tool's output with the PARENT commit's library (never
regenerated from the tree under test).
  python tools/cornell_start_digest.py [out.json]      (default: stdout)"""
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

V_INTERP = 0x2808  # FT_LIN | FT_INST | FT_BIASED, no shape id: the linear-program interpreter

# (name, scene, width, height, spp, chunk_samples or 0, MRT_NO_SIG)
_SHARED = [
    ("lens_shutter", "lens", 32, 32, 9, 0),
    ("paths_1", 5, 1, 1, 1, 0),
    ("paths_63", 5, 9, 7, 1, 0),
    ("paths_64", 5, 8, 8, 1, 0),
    ("paths_65", 5, 13, 5, 1, 0),
    ("paths_129", 5, 43, 3, 1, 0),
    ("chunked", 5, 32, 32, 16, 5),
]
CASES = [("sphere_lambertian", "lambsphere", 48, 48, 9, 0, False)] + [c + (False,) for c in _SHARED] + \
        [("nosig_" + c[0],) + c[1:] + (True,) for c in _SHARED]


def lambsphere_scene(mrt, aspect=1.0):
    from synth_scenes import Synth
    s = Synth(mrt.select_scene(5, aspect))
    s.nodes[fpd.C_SPHERE]["mat"] = s.lambertian(0.7, 0.4, 0.2)
    s._view = None
    return s


def lens_scene(mrt, aspect=1.0):
    from synth_scenes import Synth
    s = Synth(mrt.select_scene(5, aspect))
    s.camera.lens_radius = 12.0  # (the room is 555 wide)
    s.camera.time0, s.camera.time1 = 0.25, 0.75
    s._view = None
    return s


def scene_of(mrt, sid, aspect):
    if sid == "lambsphere":
        return lambsphere_scene(mrt, aspect)
    if sid == "lens":
        return lens_scene(mrt, aspect)
    return mrt.select_scene(sid, aspect)


def digest_case(mrt, case):
    name, sid, w, h, spp, chunk, nosig = case
    old = os.environ.get("MRT_NO_SIG")
    try:
        if nosig:
            os.environ["MRT_NO_SIG"] = "1"  # read at upload
        r = mrt.Renderer(scene_of(mrt, sid, w / h), 0)
    finally:
        if nosig:
            if old is None:
                del os.environ["MRT_NO_SIG"]
            else:
                os.environ["MRT_NO_SIG"] = old
    if chunk:
        img, total = r.render(mrt.render_desc(w, h, spp, numerics="fast", chunk_samples=chunk))
        out = {"image_sha256": hashlib.sha256(np.ascontiguousarray(img).view(np.uint32).tobytes()).hexdigest()}
    else:
        rgb, rays, total, _ = fpd.render_paths(mrt, r, w, h, spp)
        assert int(rays.sum()) == total, (name, int(rays.sum()), total)
        out = {"radiance_sha256": hashlib.sha256(np.ascontiguousarray(rgb).view(np.uint32).tobytes()).hexdigest(),
               "rays_sha256": hashlib.sha256(np.ascontiguousarray(rays).tobytes()).hexdigest()}
    ki = r.kernel_info()
    r.close()
    out.update({"rays": int(total), "kernel_features": int(ki["kernel_features"])})
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
