"""Shared helpers for the parity tests (scene construction identical for oracle and HIP path)."""
import numpy as np

import synth


def default_camera(mod, width=1920, height=1080, eye=(0, 0, 0), target=(0, 0, -1), vfov_deg=60.0,
                   near=0.1, far=100.0):
    """mod is either the oracle binding or the product package (same look-at helper on both)."""
    return mod.camera_look_at(eye, target, (0, 1, 0), float(np.deg2rad(vfov_deg)), width, height,
                              near, far)


def copy_camera(src, dst_cls):
    """Copy a camera struct field by field between the oracle's and the product's ctypes types so
    that both paths see bit-identical uniforms."""
    dst = dst_cls()
    for name, _ in src._fields_:
        v = getattr(src, name)
        if hasattr(v, "__len__"):
            getattr(dst, name)[:] = list(v)
        else:
            setattr(dst, name, v)
    return dst


def bits(a):
    """the uint32 view of a float32 (or uint32) array: what "bit for bit" compares"""
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def band_rows(band, H):
    """pixel rows [y0, y1) of a band of tile rows (None: the whole image)"""
    return (0, H) if band is None else (band[0] * 16, min(band[1] * 16, H))


POISON = np.float32(-7.0)            # what the frame tests pre-fill an image with


def capacity_for(d):
    """gsp::capacity_for (wgpu-3dgs-core_amd/csrc/gs_policy.h), restated: the pair capacity for a frame expected to produce
    d pairs — 25 % head room and a floor of 65536"""
    return d + d // 4 + 65536


def deep_scene(n, first=4242, opacity=250, scale=3.5):
    """layers of nearly opaque splats: most tiles are finished long before their lists end"""
    g = synth.scene(n, first=first)
    g["color"][:, 3] = opacity
    g["scale"] *= np.float32(scale)
    return g


# scenes of the two-round count tests (tests/test_gpu_round_counts.py asserts what their round 1 finishes and round 2 drops):
# opaque splats that cover a 330 x 200 view partly after the nearest few thousand, and sparse ones that need 16 384 to
# finish a single 16 x 16 tile
ROUNDS_MIXED_SCENE = dict(n=40000, first=77, opacity=255, scale=5.0)
ROUNDS_ONE_TILE_SCENE = dict(n=60000, first=123, opacity=250, scale=1.5)
_small_image_scenes = {}


def small_image_scene(W, H):
    """the Gaussians tests/test_gpu_rounds.py renders at its small sizes: a scene whose round 1 finishes some tiles and leaves
    others open — at one tile, where that cannot be, nothing at K = 2 048 and everything at 16 384"""
    spec = ROUNDS_ONE_TILE_SCENE if (W, H) == (16, 16) else ROUNDS_MIXED_SCENE
    key = tuple(sorted(spec.items()))
    if key not in _small_image_scenes:
        _small_image_scenes[key] = deep_scene(spec["n"], first=spec["first"], opacity=spec["opacity"], scale=spec["scale"])
    return _small_image_scenes[key]


def pair_walk(k):
    """A sequence over range(k), k * k + 1 long, in which every ordered pair (a, b), a == b included, occurs as two
    consecutive elements exactly once: the de Bruijn sequence B(k, 2) (concatenated Lyndon words whose length divides 2,
    in lexicographic order), closed by repeating its first element."""
    seq, a = [], [0, 0, 0]

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)
    db(1, 1)
    return seq + seq[:1]


def consecutive_pairs(seq):
    return set(zip(seq[:-1], seq[1:]))


def synth_pods(ob, sh, cov, n, first=0):
    g = synth.scene(n, first=first)
    return g, ob.pack(sh, cov, g)


def needle_gaussian(mod, theta_deg, sigma_px, opacity_byte, center_px, width, height, z=4.0, thin=1e-4):
    """One splat that projects to a needle: standard deviation `sigma_px` pixels along a direction
    `theta_deg` from the image x axis, far thinner than a pixel across (the +0.3 dilation of DESIGN.md
    §3.3 then sets the width), centred on `center_px` — cond(cov2d) = sigma_px^2 / 0.3.  Returns
    (gaussians[1], camera of `mod`)."""
    cam = default_camera(mod, width, height)
    g = synth.scene(1)
    g["sh"][:] = 0
    g["color"][0] = (200, 120, 40, opacity_byte)
    mx, my = center_px
    g["pos"][0] = ((mx - cam.cx) / cam.fx * z, -(my - cam.cy) / cam.fy * z, -z)
    g["scale"][0] = (sigma_px * z / cam.fx, thin, thin)
    t = np.deg2rad(theta_deg) / 2
    g["rot"][0] = (0.0, 0.0, np.sin(t), np.cos(t))
    return g, cam
