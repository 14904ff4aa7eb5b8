"""numpy model of gs_image_compare, operation by operation, and a float64 witness of its SSIM.

It shares no code with the library.  Every binary32 step is one numpy float32 operation (numpy rounds each of them and
fuses nothing); the sums are math.fsum of the exactly widened terms."""
import math

import numpy as np

f32 = np.float32
R = 5      # the window is 11 x 11

# the bits include/gs3d.h and the kernel header tabulate
WEIGHT_HEX = ["0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c4p-3", "0x1.10656p-2",
              "0x1.b43c4p-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d956cp-10"]

# The model against the witness on image_set(): the largest values the committed model shows (seed 20: 3.042e-4 per pixel
# at 130 x 257 and 2.394e-6 in a channel mean at 100 x 37, both on the near-constant pair, where eaa - maa cancels; every
# other pair stays below 1.5e-5 and 1.6e-7), and the bounds tests/test_metrics_api.py asserts: 4 times them, so that they
# hold for other seeds of the same generators (seeds 21 and 22 show 3.2e-4 and 3.9e-6).
MEASURED_PIXEL_DEV = 3.042e-4
MEASURED_MEAN_DEV = 2.394e-6
PIXEL_BOUND = 4 * MEASURED_PIXEL_DEV
MEAN_BOUND = 4 * MEASURED_MEAN_DEV

SIZES = [(1, 1), (5, 7), (11, 11), (16, 16), (33, 17), (100, 37), (130, 257)]      # H x W
PAIRS = ["equal", "noise", "independent", "near_constant", "sine", "out_of_range"]


def weights64():
    k = np.arange(11, dtype=np.float64)
    w = np.exp(-((k - 5.0) ** 2) / 4.5)
    return w / w.sum()


def weights():
    """g[0..10] in binary32, from the formula; the same bits as the table"""
    g = weights64().astype(f32)
    assert [float(v) for v in g] == [float.fromhex(h) for h in WEIGHT_HEX]
    return g


def image_pair(kind, h, w, seed=20):
    """(a, b): two H x W x 4 float32 images, all four channels filled"""
    rng = np.random.default_rng([seed, PAIRS.index(kind), h, w])
    a = rng.random((h, w, 4), dtype=f32)
    if kind == "equal":
        b = a.copy()
    elif kind == "noise":
        b = a + (f32(0.02) * rng.standard_normal((h, w, 4), dtype=f32))
    elif kind == "independent":
        b = rng.random((h, w, 4), dtype=f32)
    elif kind == "near_constant":
        a = f32(0.7) + f32(1e-3) * rng.standard_normal((h, w, 4), dtype=f32)
        b = f32(0.7) + f32(1e-3) * rng.standard_normal((h, w, 4), dtype=f32)
    elif kind == "sine":
        y, x = np.mgrid[0:h, 0:w].astype(f32)
        ph = np.array([0.0, 0.7, 1.9, 2.6], f32)
        a = (f32(0.5) + f32(0.5) * np.sin(f32(0.37) * x[..., None] + f32(0.23) * y[..., None] + ph)).astype(f32)
        b = f32(0.9) * a + f32(0.05)
    elif kind == "out_of_range":
        a = (f32(3.0) * a - f32(1.0)).astype(f32)
        b = (a + f32(0.3) * rng.standard_normal((h, w, 4), dtype=f32)).astype(f32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)


def image_set(seed=20):
    for h, w in SIZES:
        for kind in PAIRS:
            yield (h, w, kind) + image_pair(kind, h, w, seed)


def _filter_axis(v, g, axis):
    """acc = +0; acc = acc + g[k] v[i + k - 5], k ascending; samples outside are +0"""
    pad = [(0, 0)] * v.ndim
    pad[axis] = (R, R)
    vp = np.pad(v, pad)
    n = v.shape[axis]
    acc = np.zeros(v.shape, f32)
    for k in range(11):
        sl = [slice(None)] * v.ndim
        sl[axis] = slice(k, k + n)
        acc = acc + g[k] * vp[tuple(sl)]
    return acc


def _filter(v, g):
    return _filter_axis(_filter_axis(v, g, 1), g, 0)


def ssim_map(a, b, data_range=1.0):
    """H x W x 3 float32: the per-pixel value of each colour channel"""
    g = weights()
    a, b = a[..., :3], b[..., :3]
    L = f32(data_range)
    k1, k2 = f32(0.01) * L, f32(0.03) * L
    C1, C2 = k1 * k1, k2 * k2
    with np.errstate(all="ignore"):
        ma, mb = _filter(a, g), _filter(b, g)
        eaa, eab, ebb = _filter(a * a, g), _filter(a * b, g), _filter(b * b, g)
        maa, mbb, mab = ma * ma, mb * mb, ma * mb
        saa, sbb, sab = eaa - maa, ebb - mbb, eab - mab
        s = ((f32(2.0) * mab + C1) * (f32(2.0) * sab + C2)) / (((maa + mbb) + C1) * ((saa + sbb) + C2))
    assert s.dtype == f32
    return s


def ssim_witness(a, b, data_range=1.0):
    """float64, a direct 121-tap convolution with zero padding"""
    g = weights64()
    k2d = np.outer(g, g)
    a, b = a[..., :3].astype(np.float64), b[..., :3].astype(np.float64)
    h, w = a.shape[:2]

    def conv(v):
        vp = np.pad(v, ((R, R), (R, R), (0, 0)))
        acc = np.zeros_like(v)
        for dy in range(11):
            for dx in range(11):
                acc += k2d[dy, dx] * vp[dy:dy + h, dx:dx + w]
        return acc

    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ma, mb = conv(a), conv(b)
    saa, sbb, sab = conv(a * a) - ma * ma, conv(b * b) - mb * mb, conv(a * b) - ma * mb
    return ((2 * ma * mb + C1) * (2 * sab + C2)) / ((ma * ma + mb * mb + C1) * (saa + sbb + C2))


def compare(a, b, ssim=False, data_range=1.0):
    """the fields of gs_image_metrics and the two planes, as a dict; abs_* are the sums of |term| for the bounds of the tests"""
    h, w = a.shape[:2]
    assert a.shape == b.shape == (h, w, 4) and a.dtype == b.dtype == f32
    A, B = a.reshape(-1, 4), b.reshape(-1, 4)
    fin = np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1)
    with np.errstate(all="ignore"):
        d = A - B
    ad = np.abs(d)
    out = {"pixels": h * w, "finite": int(fin.sum()), "differing": int((fin & (d != 0).any(axis=1)).sum()),
           "bit_differing": int((A.view(np.uint32) != B.view(np.uint32)).any(axis=1).sum())}
    d64, ad64 = d[fin].astype(np.float64), ad[fin].astype(np.float64)
    out["sum_sq"] = np.array([math.fsum(d64[:, c] * d64[:, c]) for c in range(4)])      # the square of a binary32 is exact in binary64
    out["sum_abs"] = np.array([math.fsum(ad64[:, c]) for c in range(4)])
    out["abs_sq"], out["abs_abs"] = out["sum_sq"].copy(), out["sum_abs"].copy()
    out["max_abs"] = np.zeros(4, f32)
    out["max_abs_at"] = np.full(4, 0xFFFFFFFF, np.uint32)
    idx = np.flatnonzero(fin)
    if len(idx):
        for c in range(4):
            col = ad[fin, c]
            out["max_abs"][c] = col.max()
            out["max_abs_at"][c] = idx[int(np.argmax(col))]      # argmax: the first of equal maxima
    err = ad[:, 0]
    for c in range(1, 4):
        err = np.fmax(err, ad[:, c])
    err = np.where(fin, err, f32(np.nan)).astype(f32)
    err.view(np.uint32)[~fin] = 0x7FC00000
    out["err_plane"] = err.reshape(h, w)
    out["ssim_sum"], out["abs_ssim"], out["ssim_finite"] = np.zeros(3), np.zeros(3), np.zeros(3, np.uint64)
    if ssim:
        s = ssim_map(a, b, data_range)
        for c in range(3):
            v = s[..., c].ravel()
            v = v[np.isfinite(v)].astype(np.float64)
            out["ssim_sum"][c], out["abs_ssim"][c], out["ssim_finite"][c] = math.fsum(v), math.fsum(np.abs(v)), len(v)
        with np.errstate(all="ignore"):
            out["ssim_plane"] = ((s[..., 0] + s[..., 1]) + s[..., 2]) / f32(3.0)
        out["ssim_map"] = s
    return out
