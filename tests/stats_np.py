"""numpy restatement of DESIGN.md §3.10 (attributes, their statistics, histograms and range select), written from the text:
every operation is one rounded float32 operation in the written order, min and max go through the sortable integer of the
bit pattern, the sum is math.fsum (exact, rounded once).  Shares no code with the library."""
import math

import numpy as np

import edit_np

f32 = np.float32
X, Y, Z, RED, GREEN, BLUE, OPACITY, SIZE2, DIST2 = range(9)
ATTR_COUNT = 9
IDENTITY = dict(pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0, 1.0), scale=(1.0, 1.0, 1.0))


def world_positions(x, pos, rot, scale):
    """pw = M (p, 1), ((c0 + c1) + c2) + c3; the default transform goes through the same arithmetic (inf 0 = NaN)"""
    A = edit_np.scale_rot_mat(rot, scale)
    t = np.asarray(pos, f32)
    return np.stack([((A[k, 0] * x[:, 0] + A[k, 1] * x[:, 1]) + A[k, 2] * x[:, 2]) + t[k] for k in range(3)], axis=1)


def cov_diagonal(cov, raw):
    """raw: n x COV_BYTES uint8 -> (S00, S11, S22) of the layout's decoded 3D covariance"""
    n = raw.shape[0]
    if cov == 1:
        c6 = np.ascontiguousarray(raw[:, :24]).view(f32).reshape(n, 6)
        return c6[:, 0], c6[:, 3], c6[:, 5]
    if cov == 2:
        c6 = np.ascontiguousarray(raw[:, :12]).view(np.float16).reshape(n, 6).astype(f32)
        return c6[:, 0], c6[:, 3], c6[:, 5]
    c = np.ascontiguousarray(raw[:, :28]).view(f32).reshape(n, 7)
    rx, ry, rz, rw, sx, sy, sz = [c[:, k] for k in range(7)]
    one = f32(1.0)
    x2, y2, z2 = rx + rx, ry + ry, rz + rz
    xx, xy, xz = rx * x2, rx * y2, rx * z2
    yy, yz, zz = ry * y2, ry * z2, rz * z2
    wx, wy, wz = rw * x2, rw * y2, rw * z2
    m0 = [(one - (yy + zz)) * sx, (xy + wz) * sx, (xz - wy) * sx]
    m1 = [(xy - wz) * sy, (one - (xx + zz)) * sy, (yz + wx) * sy]
    m2 = [(xz + wy) * sz, (yz - wx) * sz, (one - (xx + yy)) * sz]
    return tuple((m0[k] * m0[k] + m1[k] * m1[k]) + m2[k] * m2[k] for k in range(3))


def attributes(sh, cov, rows, pos=IDENTITY["pos"], rot=IDENTITY["rot"], scale=IDENTITY["scale"], ref=(0.0, 0.0, 0.0)):
    """rows: n x pod_bytes uint8 -> n x 9 float32, column k = attribute k"""
    rows = np.asarray(rows, np.uint8).reshape(-1, edit_np.pod_bytes(sh, cov))
    n = rows.shape[0]
    out = np.zeros((n, ATTR_COUNT), f32)
    with np.errstate(all="ignore"):
        x = np.ascontiguousarray(rows[:, 0:12]).view(f32).reshape(n, 3)
        pw = world_positions(x, pos, rot, scale)
        out[:, X:Z + 1] = pw
        out[:, RED:OPACITY + 1] = rows[:, 12:16].astype(f32) / f32(255.0)
        cov0 = 16 + edit_np.SH_BYTES[sh]
        s00, s11, s22 = cov_diagonal(cov, rows[:, cov0:cov0 + edit_np.COV_BYTES[cov]])
        out[:, SIZE2] = (s00 + s11) + s22
        d = pw - np.asarray(ref, f32)[None, :]
        out[:, DIST2] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return out


def sort_keys(v):
    """the total order on the bit patterns as unsigned integers: -0 < +0"""
    u = np.ascontiguousarray(v, f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(key):
    key = np.uint32(key)
    u = key ^ np.uint32(0x80000000) if key & np.uint32(0x80000000) else ~key
    return np.array([u], np.uint32).view(f32)[0]


def stats(values, mask=None):
    """values: n x 9 float32.  Returns dict(count, finite uint64[9], min f32[9], max f32[9], sum f64[9] (math.fsum),
    abs_sum f64[9] (math.fsum of |v|, for the bound on the device's sum))."""
    n = values.shape[0]
    m = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    out = dict(count=int(m.sum()), finite=np.zeros(ATTR_COUNT, np.uint64), min=np.full(ATTR_COUNT, np.inf, f32),
               max=np.full(ATTR_COUNT, -np.inf, f32), sum=np.zeros(ATTR_COUNT, np.float64), abs_sum=np.zeros(ATTR_COUNT, np.float64))
    for k in range(ATTR_COUNT):
        v = values[m, k]
        v = v[np.isfinite(v)]
        out["finite"][k] = len(v)
        if len(v):
            keys = sort_keys(v)
            out["min"][k] = key_to_float(keys.min())
            out["max"][k] = key_to_float(keys.max())
            out["sum"][k] = math.fsum(float(x) for x in v)
            out["abs_sum"][k] = math.fsum(abs(float(x)) for x in v)
    return out


def histogram_slots(v, lo, hi, bins):
    """slot of every value: NaN -> bins + 2, v < lo -> bins, v >= hi -> bins + 1, else trunc((v - lo) scale) clamped"""
    v = np.asarray(v, f32)
    lo, hi = f32(lo), f32(hi)
    scale = f32(bins) / (hi - lo)
    assert np.isfinite(scale)
    with np.errstate(all="ignore"):
        b = np.minimum(((v - lo) * scale).astype(np.float64), float(bins - 1))
        b = np.where(np.isfinite(b), b, 0.0).astype(np.int64)       # (overwritten below wherever v is out of range)
        slot = np.where(np.isnan(v), bins + 2, np.where(v < lo, bins, np.where(v >= hi, bins + 1, b)))
    return slot.astype(np.int64)


def histogram(v, lo, hi, bins, mask=None):
    """uint64[2, bins + 3]: row 0 the masked values (None: all), row 1 the others"""
    slots = histogram_slots(v, lo, hi, bins)
    m = np.ones(len(slots), bool) if mask is None else np.asarray(mask, bool)
    return np.stack([np.bincount(slots[m], minlength=bins + 3), np.bincount(slots[~m], minlength=bins + 3)]).astype(np.uint64)


def in_range(v, lo, hi):
    """{i : lo <= v_i && v_i <= hi}; NaN compares false"""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        return (f32(lo) <= v) & (v <= f32(hi))


def pack_bits(flags):
    a = np.packbits(np.asarray(flags, bool), bitorder="little")
    return np.concatenate([a, np.zeros(-len(a) % 4, np.uint8)]).view(np.uint32)
