#!/usr/bin/env python3
"""Digests of the Cornell kernels' per-path results on the cases that matter once the light's extents
and area (b1 - b0, b3 - b2 and their product: constants of a launch) are computed once per wave and
read from its LDS by the light sampling and the light pdf, the pdf's cosine is |d.y * ns|, and the
forward fold of a diffuse scatter under the walk's light has no "no pdf" side.  Every path keeps its
operations' values, their order and its stream positions.

  s5                  scene 5 at 64x64x16, depth limit 32
  s5_dD               depth limits D = 1, 2 at 16x16x4
  paths_N             scene 5 with N = 1, 63, 64, 65 paths at 1 spp
  light_*             scene 5 with other words in the light's rect (op 3, which is the biased leaf):
                        uneven   40 x 210
                        corner   the stock size moved towards a corner of the ceiling
                        unit     one unit wide (its area is its other extent)
                        inexact  bounds whose float32 differences round (101.1 .. 343.7, 90.1 .. 332.9)
  offlight            another rect as the biased object: the pdf takes the leaf path, nothing of the quad is used
  alt                 two renderers with different lights (uneven, inexact) on ONE device, rendered a, b, a:
                      each render's digests in order; the first and third must agree
  glass               the glass-heavy scene: all 64 lanes take the glass branch
  nosig_s5            s5_d2's render through the interpreter's queue kernel (MRT_NO_SIG=1)

LIGHTS holds each test light's (x0, x1, z0, z1); light_words() the float32 words the kernel is given.
tools/fast_path_digest.py's method: numerics="fast", MRT_RF_PATH_DEBUG (the per-path ray count is
stored beside the radiance), sha256 of the per-path radiance bits and ray counts.
tests/test_cornell_light_gpu.py compares with the committed tests/golden/cornell_light_parent.json, this
tool's output with the PARENT commit's library (never regenerated from the tree under test).
  python tools/cornell_light_digest.py [out.json]      (default: stdout)"""
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
C_LIGHT = 3  # scene 5's view: the light's node (the program's op 3, the biased list's one leaf)
# the test lights' bounds (x0, x1, z0, z1) inside the 555 x 555 ceiling; "stock" is scene 5's own
LIGHTS = {"stock": (213.0, 343.0, 227.0, 332.0),
          "uneven": (260.0, 300.0, 170.0, 380.0),
          "corner": (20.0, 150.0, 400.0, 505.0),
          "unit": (277.0, 278.0, 227.0, 332.0),
          "inexact": (101.1, 343.7, 90.1, 332.9)}


def light_words(name):
    """The light's bounds as the float32 words the scene holds."""
    return np.asarray(LIGHTS[name], dtype=np.float32)


def light_scene(mrt, name, aspect=1.0):
    """Scene 5 with the light's rect (and the biased list's box around it) on LIGHTS[name]'s bounds."""
    from synth_scenes import K_LIST, K_XZ, Synth
    s = Synth(mrt.select_scene(5, aspect))
    lamp = s.nodes[C_LIGHT]
    assert (int(lamp["kind"]) & 0xFF) == K_XZ
    b = light_words(name)
    if name == "stock":
        assert np.array_equal(lamp["f"][:4], b), lamp["f"][:4]
        return s
    lamp["f"][:4] = b
    bl = s.nodes[s.biased]
    assert (int(bl["kind"]) & 0xFF) == K_LIST and s.list_items(int(s.biased)) == [C_LIGHT]
    y = float(lamp["f"][4])
    bl["f"][:6] = np.asarray((b[0], y - 0.0001, b[2], b[1], y + 0.0001, b[3]), dtype=np.float32)
    s._view = None
    return s


def scene_of(mrt, sid, aspect):
    if isinstance(sid, str) and sid.startswith("light_"):
        return light_scene(mrt, sid[len("light_"):], aspect)
    return crd.scene_of(mrt, sid, aspect)


_PATHS = {1: (1, 1), 63: (9, 7), 64: (8, 8), 65: (13, 5)}
# (name, scenes of the renderers, width, height, spp, renders as (renderer, depth limit) in order, MRT_NO_SIG)
CASES = [("s5", (5,), 64, 64, 16, ((0, 32),), False),
         ("s5_d1", (5,), 16, 16, 4, ((0, 1),), False),
         ("s5_d2", (5,), 16, 16, 4, ((0, 2),), False)] + [
    (f"paths_{n}", (5,), wh[0], wh[1], 1, ((0, 32),), False) for n, wh in _PATHS.items()] + [
    (f"light_{n}", (f"light_{n}",), 24, 24, 4, ((0, 32),), False) for n in ("uneven", "corner", "unit", "inexact")] + [
    ("offlight", ("offlight",), 24, 24, 4, ((0, 32),), False),
    ("alt", ("light_uneven", "light_inexact"), 24, 24, 4, ((0, 32), (1, 32), (0, 32)), False),
    ("glass", ("glass",), 16, 16, 4, ((0, 32),), False),
    ("nosig_s5", (5,), 16, 16, 4, ((0, 2),), True)]


def n_paths(case):
    return case[2] * case[3] * case[4]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest_case(mrt, case):
    name, sids, w, h, spp, renders, nosig = case
    old = os.environ.get("MRT_NO_SIG")
    try:
        if nosig:
            os.environ["MRT_NO_SIG"] = "1"  # read at upload
        rs = [mrt.Renderer(scene_of(mrt, sid, w / h), 0) for sid in sids]
    finally:
        if nosig:
            if old is None:
                del os.environ["MRT_NO_SIG"]
            else:
                os.environ["MRT_NO_SIG"] = old
    out = {"renders": []}
    for k, depth in renders:
        rgb, rays, total, _ = fpd.render_paths(mrt, rs[k], w, h, spp, depth)
        assert int(rays.sum()) == total, (name, int(rays.sum()), total)
        out["renders"].append({"radiance_sha256": _sha(np.ascontiguousarray(rgb).view(np.uint32)), "rays_sha256": _sha(rays),
                               "renderer": k, "depth": depth, "rays": int(total)})
    out["kernel_features"] = [int(r.kernel_info()["kernel_features"]) for r in rs]
    for r in rs:
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
