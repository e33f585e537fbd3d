#!/usr/bin/env python3
"""Digests of the tolerance contract's per-path results: for a fixed list of cases, rendered with
numerics="fast" and MRT_RF_PATH_DEBUG (one launch, no hand-over: the fast kernel's own radiance), the
sha256 of the per-path radiance bits, the sha256 of the per-path ray counts (both in stream order,
path k = pixel * ns + s) and the ray total.  A change that only reschedules the path kernel's work
leaves every digest as it was (tests/test_parked_scatter.py compares with the committed
tests/golden/fastpaths_parent.json).
  python tools/fast_path_digest.py [out.json]      (default: stdout)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (name, scene, width, height, spp, depth, mode); scenes "glass" / "offlight": glass_scene() / offlight_scene() below
CASES = [
    ("s5_64x64x16", 5, 64, 64, 16, 32, 0),
    ("s5_48x48x4_depth1", 5, 48, 48, 4, 1, 0),
    ("s5_48x48x4_depth2", 5, 48, 48, 4, 2, 0),
    ("s5_33x31x9", 5, 33, 31, 9, 32, 0),
    ("s5_7x5x1", 5, 7, 5, 1, 32, 0),
    ("s5_1x1x1", 5, 1, 1, 1, 32, 0),
    ("s5_64x64x16_mode1", 5, 64, 64, 16, 32, 1),
    ("glass_64x64x16", "glass", 64, 64, 16, 32, 0),
    ("glass_16x16x4", "glass", 16, 16, 4, 32, 0),
    ("offlight_48x48x4", "offlight", 48, 48, 4, 32, 0),
]
# scene 5's view: root list 0, glass sphere node 16 (tests/test_synthetic_scenes.py)
C_ROOT, C_SPHERE = 0, 16
V_CORNELL = 0x1 << 16 | 0x2808  # FT_LIN | FT_INST | FT_BIASED | SIG_CORNELL


def glass_scene(mrt, aspect=1.0):
    """The Cornell signature with the glass sphere moved onto the view axis, between the camera and
    the room, and enlarged until it covers the whole image: every camera ray meets glass first (every
    lane of a wave at once), and paths bounce inside the sphere (one path meets glass many times
    running).  The root list's box grows to hold it."""
    from synth_scenes import Synth
    s = Synth(mrt.select_scene(5, aspect))
    cam = s.camera
    # 500 in front of the camera; the image's corner is tan(20 deg) * sqrt(1 + aspect^2) off the axis
    f = s.nodes[C_SPHERE]["f"]
    f[0], f[1], f[2] = cam.origin[0], cam.origin[1], cam.origin[2] + 500.0
    f[8] = 250.0
    box = s.nodes[C_ROOT]["f"]
    box[2] = min(box[2], f[2] - f[8] - 1.0)
    s._view = None
    return s


def offlight_scene(mrt, aspect=1.0):
    """Scene 5 with another xz_rect as the biased object: narrower than the light (op 3) and not in
    the scene graph.  Same kernel; the light pdf cannot come from the walk's light test here
    (DScene::light_once off), so the kernel's biased_pdf_value branch runs."""
    from synth_scenes import K_XZ, Synth
    s = Synth(mrt.select_scene(5, aspect))
    lamp = s.nodes[3]
    other = s.rect(K_XZ, 240.0, 330.0, 250.0, 310.0, float(lamp["f"][4]), int(lamp["mat"]), float(lamp["f"][5]))
    s.biased = s.list([other], box=(240.0, 553.9999, 250.0, 330.0, 554.0001, 310.0))
    return s


def scene_of(mrt, sid, aspect):
    if sid == "glass":
        return glass_scene(mrt, aspect)
    if sid == "offlight":
        return offlight_scene(mrt, aspect)
    return mrt.select_scene(sid, aspect)


def stream_order(mrt, r, d, w, h):
    """Per-path radiance (w*h, ns, 3) and rays (w*h, ns) of the debug render just made with d, the
    pixels d does not render left zero; + the pixels it rendered."""
    ns = d.sqrt_samples ** 2
    px = mrt.local_pixels(d)
    prgb, prays = r.paths(len(px) * ns)
    rgb = np.zeros((w * h, ns, 3), dtype=np.float32)
    rays = np.zeros((w * h, ns), dtype=np.uint32)
    rgb[px] = prgb.reshape(ns, len(px), 3).transpose(1, 0, 2)
    rays[px] = prays.reshape(ns, len(px)).T
    return rgb, rays, px


def render_paths(mrt, r, w, h, spp, depth=32, mode=0, **kw):
    d = mrt.render_desc(w, h, spp, depth=depth, mode=mode, numerics="fast", flags=mrt._lib.RF_PATH_DEBUG, **kw)
    _, total = r.render(d)
    rgb, rays, px = stream_order(mrt, r, d, w, h)
    return rgb, rays, total, px


def digest_case(mrt, case):
    name, sid, w, h, spp, depth, mode = case
    r = mrt.Renderer(scene_of(mrt, sid, w / h), 0)
    rgb, rays, total, _ = render_paths(mrt, r, w, h, spp, depth, mode)
    ki = r.kernel_info()
    r.close()
    assert int(rays.sum()) == total, (name, int(rays.sum()), total)
    return {"radiance_sha256": hashlib.sha256(np.ascontiguousarray(rgb).view(np.uint32).tobytes()).hexdigest(),
            "rays_sha256": hashlib.sha256(np.ascontiguousarray(rays).tobytes()).hexdigest(),
            "rays": int(total), "kernel_features": int(ki["kernel_features"])}


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
