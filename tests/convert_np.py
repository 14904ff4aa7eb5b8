"""numpy restatement of DESIGN.md §3.12 (conversion of records between the 12 layouts), written from the text: a section
whose config is kept is copied, any other is decoded and encoded again, every pad is zero.  The f16 steps are numpy's
astype (round to nearest even, exact the other way); NaNs are covered as far as numpy's conversions and the library's agree:
quiet NaNs, which is all that packing np.nan produces.  Shares no code with the library."""
import numpy as np

from edit_np import COV_BYTES, SH_BYTES, decode_sh, encode_sh, pod_bytes, quat_terms

f32 = np.float32


def convertible(ssh, scov, dsh, dcov):
    return dcov != 0 or scov == 0


def canon_bits(a):
    """binary32 values -> their bits, a computed NaN as +qNaN"""
    a = np.ascontiguousarray(a, dtype=f32)
    bits = a.view(np.uint32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return bits


def cov_from_rot_scale(c):
    """c: n x 7 float32 (rot xyzw, scale) -> n x 6 float32, (R S)(R S)^T, each sum ((k0 + k1) + k2)"""
    t = quat_terms([c[:, 0], c[:, 1], c[:, 2], c[:, 3]])
    sx, sy, sz = c[:, 4], c[:, 5], c[:, 6]
    one = f32(1.0)
    # A[r][k]: column k of the rotation matrix scaled by s_k
    A = [[(one - (t["yy"] + t["zz"])) * sx, (t["xy"] - t["wz"]) * sy, (t["xz"] + t["wy"]) * sz],
         [(t["xy"] + t["wz"]) * sx, (one - (t["xx"] + t["zz"])) * sy, (t["yz"] - t["wx"]) * sz],
         [(t["xz"] - t["wy"]) * sx, (t["yz"] + t["wx"]) * sy, (one - (t["xx"] + t["yy"])) * sz]]

    def sig(r, k):
        return (A[r][0] * A[k][0] + A[r][1] * A[k][1]) + A[r][2] * A[k][2]
    return np.stack([sig(0, 0), sig(1, 0), sig(2, 0), sig(1, 1), sig(2, 1), sig(2, 2)], axis=1).astype(f32)


def convert(ssh, scov, dsh, dcov, pods):
    """pods: uint8, n records of layout (ssh, scov) -> uint8, n records of layout (dsh, dcov)"""
    assert convertible(ssh, scov, dsh, dcov)
    sb, db = pod_bytes(ssh, scov), pod_bytes(dsh, dcov)
    p = np.asarray(pods, dtype=np.uint8).reshape(-1, sb)
    if (ssh, scov) == (dsh, dcov):       # identical layouts keep every byte
        return p.reshape(-1).copy()
    n = p.shape[0]
    out = np.zeros((n, db), np.uint8)
    out[:, :16] = p[:, :16]
    s_sh, d_sh = p[:, 16:16 + SH_BYTES[ssh]], out[:, 16:16 + SH_BYTES[dsh]]
    with np.errstate(all="ignore"):
        if dsh == ssh:
            d_sh[:] = s_sh
        elif dsh != 3:
            c = decode_sh(ssh, s_sh) if ssh != 3 else np.zeros((n, 45), f32)
            if dsh == 0:
                d_sh[:] = np.ascontiguousarray(c).view(np.uint8).reshape(n, 180)
            elif dsh == 1:
                d_sh[:, :90] = c.astype(np.float16).view(np.uint8).reshape(n, 90)
            else:
                d_sh[:] = encode_sh(2, c)
        s_cov = np.ascontiguousarray(p[:, 16 + SH_BYTES[ssh]:16 + SH_BYTES[ssh] + COV_BYTES[scov]])
        d_cov = out[:, 16 + SH_BYTES[dsh]:16 + SH_BYTES[dsh] + COV_BYTES[dcov]]
        if dcov == scov:
            d_cov[:] = s_cov
        else:
            if scov == 0:
                bits = canon_bits(cov_from_rot_scale(s_cov.view(f32).reshape(n, 7)))
            elif scov == 1:
                bits = s_cov.view(np.uint32).reshape(n, 6)
            else:
                bits = s_cov.view(np.float16).reshape(n, 6).astype(f32).view(np.uint32)
            if dcov == 1:
                d_cov[:] = np.ascontiguousarray(bits).view(np.uint8).reshape(n, 24)
            else:
                d_cov[:] = np.ascontiguousarray(bits).view(f32).astype(np.float16).view(np.uint8).reshape(n, 12)
    return out.reshape(-1)
