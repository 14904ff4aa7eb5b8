"""Covariance -> rotation + scale: the inputs the decomposition tests share and a float64 witness that is
independent of the code under test (numpy.linalg.eigh on the binary32 inputs, negative eigenvalues clamped at 0).
Everything cached here is read-only."""
import numpy as np

import synth

f32 = np.float32
COV_WORDS = ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))      # (row, column) of the six terms xx, yx, zx, yy, zy, zz


# ---- the set ---------------------------------------------------------------------------------------------------------

def set_gaussians(n, seed=11):
    """n Gaussians with random rotations and scales log-uniform in [1e-4, 1e2]; 10 % with two equal scales, 10 % isotropic,
    5 % flat (one scale 0), 8 % with two scales a factor 1 + 1e-6 apart.  Positions, colours and SH are synth.scene's."""
    rng = np.random.default_rng(seed)
    g = synth.scene(n, first=seed)
    q = rng.standard_normal((n, 4))
    g["rot"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    s = np.exp(rng.uniform(np.log(1e-4), np.log(1e2), (n, 3)))
    kind = rng.random(n)
    two = kind < 0.10
    s[two, 1] = s[two, 0]
    iso = (kind >= 0.10) & (kind < 0.20)
    s[iso, 1] = s[iso, 0]
    s[iso, 2] = s[iso, 0]
    flat = (kind >= 0.20) & (kind < 0.25)
    s[flat, 2] = 0.0
    near = (kind >= 0.25) & (kind < 0.33)
    s[near, 1] = s[near, 0] * (1.0 + 1e-6)
    g["scale"] = s.astype(f32)
    return g


def raw_symmetric(n, seed=12):
    """(n, 6) binary32: symmetric matrices with entries uniform in [-1, 1], indefinite on purpose"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 6)).astype(f32)


def cov_words(gs, pods, sh, cov):
    """(n, 6) binary32: the covariance terms of packed records of a covariance layout, f16 decoded exactly"""
    pod = gs.GaussianPod(sh, cov)
    rows = np.ascontiguousarray(pods).reshape(-1, pod.size)
    at = 16 + (180, 92, 48, 0)[sh]
    if cov == 1:
        return np.ascontiguousarray(rows[:, at:at + 24]).view(f32).copy()
    return np.ascontiguousarray(rows[:, at:at + 12]).view(np.float16).astype(f32)


def cov_records(c6):
    """(n, 6) binary32 -> packed SH-less cov-f32 records (48 bytes: position 0, colour 0xff, the six words, zero pad)"""
    c6 = np.ascontiguousarray(c6, f32).reshape(-1, 6)
    rows = np.zeros((len(c6), 48), np.uint8)
    rows[:, 12:16] = 0xFF
    rows[:, 16:40] = c6.view(np.uint8)
    return rows.reshape(-1)


_SET = {}


def the_set(gs, n=20000, nraw=2000):
    """{"g": the Gaussians, "f32": (n + nraw, 6) covariances of the cov-f32 records of gs_pack followed by the raw matrices,
    "f16": (n, 6) covariances of the cov-f16 records of gs_pack, decoded}: once per size, read-only"""
    key = (n, nraw)
    if key not in _SET:
        g = set_gaussians(n)
        a = cov_words(gs, gs.GaussianPod(3, 1).from_gaussian(g), 3, 1)
        h = cov_words(gs, gs.GaussianPod(3, 2).from_gaussian(g), 3, 2)
        out = {"g": g, "f32": np.concatenate([a, raw_symmetric(nraw)]), "f16": h}
        for v in out.values():
            v.setflags(write=False)
        _SET[key] = out
    return _SET[key]


def decompose_many(gs, c6):
    """gs_cov3d_decompose over (n, 6) covariances, through gs_decompose_pods on SH-less records: (rot (n, 4), scale (n, 3))"""
    out = gs.GaussianPod(3, 1).decompose(cov_records(c6), 3).reshape(-1, 48)
    return np.ascontiguousarray(out[:, 16:32]).view(f32), np.ascontiguousarray(out[:, 32:44]).view(f32)


# ---- the witness -----------------------------------------------------------------------------------------------------

def matrices(c6):
    """(n, 6) -> (n, 3, 3) float64 symmetric"""
    c6 = np.asarray(c6, np.float64).reshape(-1, 6)
    m = np.zeros((len(c6), 3, 3))
    for k, (r, c) in enumerate(COV_WORDS):
        m[:, r, c] = c6[:, k]
        m[:, c, r] = c6[:, k]
    return m


def witness(c6):
    """float64 eigen-decomposition of the binary32 inputs: (eigenvalues ascending with negatives clamped at 0 (n, 3),
    eigenvectors as columns with det +1 (n, 3, 3), the clamp residue ||min(lambda, 0)|| (n,), ||C||_F (n,))"""
    m = matrices(c6)
    lam, v = np.linalg.eigh(m)
    v[:, :, 0] *= np.sign(np.linalg.det(v))[:, None]
    return np.maximum(lam, 0.0), v, np.linalg.norm(np.minimum(lam, 0.0), axis=1), np.linalg.norm(m, axis=(1, 2))


def rotation(q):
    """unit quaternions xyzw (n, 4) -> rotation matrices (n, 3, 3), float64"""
    x, y, z, w = np.asarray(q, np.float64).reshape(-1, 4).T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def quaternion(v):
    """rotation matrices (n, 3, 3) with det +1 -> unit quaternions xyzw with w >= 0, float64 (largest-component branches)"""
    v = np.asarray(v, np.float64)
    m = lambda r, c: v[:, r, c]
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    cand = np.stack([
        np.stack([1 + m(0, 0) - m(1, 1) - m(2, 2), m(0, 1) + m(1, 0), m(0, 2) + m(2, 0), m(2, 1) - m(1, 2)], -1),
        np.stack([m(0, 1) + m(1, 0), 1 - m(0, 0) + m(1, 1) - m(2, 2), m(1, 2) + m(2, 1), m(0, 2) - m(2, 0)], -1),
        np.stack([m(0, 2) + m(2, 0), m(1, 2) + m(2, 1), 1 - m(0, 0) - m(1, 1) + m(2, 2), m(1, 0) - m(0, 1)], -1),
        np.stack([m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1), 1 + tr], -1)], 1)
    best = np.argmax(np.stack([cand[:, k, k] for k in range(4)], -1), axis=1)
    q = cand[np.arange(len(v)), best]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.where(q[:, 3:4] < 0, -q, q)


def eigenvalue_error(scale, c6):
    """max_k |scale_k^2 - lambda_k| / ||C||_F after sorting both; rows with C = 0 give 0"""
    lam, _, _, norm = witness(c6)
    s2 = np.sort(np.asarray(scale, np.float64) ** 2, axis=1)
    return np.abs(s2 - lam).max(axis=1) / np.where(norm > 0, norm, 1.0)


def reconstruction_error(recon6, c6):
    """||recon - C||_F / ||C||_F minus the witness's clamp residue ||min(lambda, 0)|| / ||C||_F; rows with C = 0 give the
    absolute error"""
    _, _, residue, norm = witness(c6)
    d = np.linalg.norm(matrices(recon6) - matrices(c6), axis=(1, 2))
    return (d - residue) / np.where(norm > 0, norm, 1.0)


def repack_cov(gs, rot, scale):
    """cov3d_from_rot_scale through gs_pack: (n, 6) binary32 covariances of the given rotations and scales"""
    g = np.zeros(len(rot), gs.GAUSSIAN_DTYPE)
    g["rot"], g["scale"] = rot, scale
    return cov_words(gs, gs.GaussianPod(3, 1).from_gaussian(g), 3, 1)


# ---- selection masks of the compaction test (those of the conversion test) -------------------------------------------

def compaction_masks(n):
    """(name, mask, invert): random 30 %, empty, all, a whole 1024-block unselected with something behind it, last only,
    inverted"""
    rng = np.random.default_rng(n)
    hole = rng.random(n) < 0.5
    hole[(n // 1024 // 2) * 1024:(n // 1024 // 2 + 1) * 1024] = False
    hole[-1] = n > 1024
    last = np.zeros(n, bool)
    last[-1] = True
    return [("random", rng.random(n) < 0.3, False), ("empty", np.zeros(n, bool), False), ("all", np.ones(n, bool), False),
            ("hole", hole, False), ("last", last, False), ("invert", rng.random(n) < 0.3, True)]
