"""numpy binary32 restatement of DESIGN.md §3.8 (edits of the selected Gaussians), written from the text: every operation
is one rounded float32 operation in the written order, so the result must equal the device's byte for byte.  Shares no
code with the library; the SH rotation matrices are an INPUT (the test takes them from gs_sh_rotation_matrices, whose
defining property tests/test_edit_api.py checks on its own)."""
import numpy as np

f32 = np.float32
SH_BYTES = [180, 92, 48, 0]        # f32, f16, snorm8, none
COV_BYTES = [28, 24, 12]           # rot + scale, six f32, six f16
TRANSFORM, ROTATE_SH, COLOR, OPACITY = 1, 2, 4, 8


def pod_bytes(sh, cov):
    return (16 + SH_BYTES[sh] + COV_BYTES[cov] + 15) // 16 * 16


def canon(a):
    """a computed NaN is stored as +qNaN (0x7fc00000)"""
    a = np.array(a, dtype=f32)
    a.view(np.uint32)[np.isnan(a)] = 0x7FC00000
    return a


def quat_terms(q):
    x, y, z, w = [f32(v) for v in q]
    x2, y2, z2 = x + x, y + y, z + z
    return dict(xx=x * x2, xy=x * y2, xz=x * z2, yy=y * y2, yz=y * z2, zz=z * z2, wx=w * x2, wy=w * y2, wz=w * z2)


def scale_rot_mat(rot, scale):
    """model_scale_rot_mat: A[r][c], the columns of the quaternion's matrix scaled"""
    t = quat_terms(rot)
    sx, sy, sz = [f32(v) for v in scale]
    one = f32(1.0)
    a = np.zeros((3, 3), f32)
    a[0, 0], a[1, 0], a[2, 0] = (one - (t["yy"] + t["zz"])) * sx, (t["xy"] + t["wz"]) * sx, (t["xz"] - t["wy"]) * sx
    a[0, 1], a[1, 1], a[2, 1] = (t["xy"] - t["wz"]) * sy, (one - (t["xx"] + t["zz"])) * sy, (t["yz"] + t["wx"]) * sy
    a[0, 2], a[1, 2], a[2, 2] = (t["xz"] + t["wy"]) * sz, (t["yz"] - t["wx"]) * sz, (one - (t["xx"] + t["yy"])) * sz
    return a


def quant_unorm(v):
    """t = v 255 + 0.5; 0 for t <= 0 or NaN, 255 for t >= 255, else floor(t)"""
    t = v.astype(f32) * f32(255.0) + f32(0.5)
    out = np.zeros(t.shape, np.uint8)
    mid = (t > 0) & (t < 255)
    out[mid] = np.floor(t[mid]).astype(np.uint8)
    out[t >= 255] = 255
    return out


def decode_sh(sh, raw):
    """raw: n x SH_BYTES uint8 -> n x 45 float32"""
    n = raw.shape[0]
    if sh == 0:
        return np.ascontiguousarray(raw[:, :180]).view(f32).reshape(n, 45).copy()
    if sh == 1:
        return np.ascontiguousarray(raw[:, :90]).view(np.float16).reshape(n, 45).astype(f32)
    b = np.ascontiguousarray(raw[:, :45]).view(np.int8).astype(f32)
    return np.maximum(b / f32(127.0), f32(-1.0))


def encode_sh(sh, c):
    """n x 45 float32 -> n x SH_BYTES uint8 (padding 0)"""
    n = c.shape[0]
    c = canon(c)
    out = np.zeros((n, SH_BYTES[sh]), np.uint8)
    if sh == 0:
        out[:, :180] = c.view(np.uint8).reshape(n, 180)
    elif sh == 1:
        out[:, :90] = c.astype(np.float16).view(np.uint8).reshape(n, 90)       # round to nearest even
    else:
        x = c * f32(127.0)
        x[np.isnan(x)] = 0
        x = np.trunc(np.clip(x, f32(-127.0), f32(127.0)))
        out[:, :45] = x.astype(np.int8).view(np.uint8)
    return out


def lin3(m, v):
    """(m0 v0 + m1 v1) + m2 v2 per row of the 3 x 3 m; v: n x 3"""
    return np.stack([(m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2] for r in range(3)], axis=1)


def apply_edit(sh, cov, pods, mask, flags, pos=(0, 0, 0), rot=(0, 0, 0, 1), scale=(1, 1, 1), color=None, opacity=None, D=None):
    """pods: uint8 (n * pod_bytes); mask: bool n or None (all).  color: 12 float32, column-major 3 x 4; opacity: (o0, o1);
    D: (D1, D2, D3) row-major.  Returns the edited bytes."""
    nb = pod_bytes(sh, cov)
    p = np.array(pods, dtype=np.uint8).reshape(-1, nb)
    n = p.shape[0]
    sel = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    r = p[sel].copy()
    if sh == 3:
        flags &= ~ROTATE_SH
    sh0, cov0 = 16, 16 + SH_BYTES[sh]
    with np.errstate(all="ignore"):
        if flags & TRANSFORM:
            A = scale_rot_mat(rot, scale)
            t = np.asarray(pos, f32)
            x = np.ascontiguousarray(r[:, 0:12]).view(f32).reshape(-1, 3)
            # M (p, 1): ((c0 + c1) + c2) + c3, M's last column = pos
            xw = np.stack([((A[k, 0] * x[:, 0] + A[k, 1] * x[:, 1]) + A[k, 2] * x[:, 2]) + t[k] for k in range(3)], axis=1)
            r[:, 0:12] = canon(xw).view(np.uint8).reshape(-1, 12)
            if cov == 0:
                c = np.ascontiguousarray(r[:, cov0:cov0 + 28]).view(f32).reshape(-1, 7)
                rx, ry, rz, rw = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
                qx, qy, qz, qw = [f32(v) for v in rot]
                out = np.empty_like(c)
                out[:, 0] = ((qw * rx + qx * rw) + qy * rz) - qz * ry
                out[:, 1] = ((qw * ry - qx * rz) + qy * rw) + qz * rx
                out[:, 2] = ((qw * rz + qx * ry) - qy * rx) + qz * rw
                out[:, 3] = ((qw * rw - qx * rx) - qy * ry) - qz * rz
                out[:, 4:7] = f32(scale[0]) * c[:, 4:7]
                r[:, cov0:cov0 + 28] = canon(out).view(np.uint8).reshape(-1, 28)
            else:
                if cov == 1:
                    c6 = np.ascontiguousarray(r[:, cov0:cov0 + 24]).view(f32).reshape(-1, 6).copy()
                else:
                    c6 = np.ascontiguousarray(r[:, cov0:cov0 + 12]).view(np.float16).reshape(-1, 6).astype(f32)
                S = [[c6[:, 0], c6[:, 1], c6[:, 2]], [c6[:, 1], c6[:, 3], c6[:, 4]], [c6[:, 2], c6[:, 4], c6[:, 5]]]
                T = [[(A[i, 0] * S[0][j] + A[i, 1] * S[1][j]) + A[i, 2] * S[2][j] for j in range(3)] for i in range(3)]
                o = np.stack([(T[i][0] * A[j, 0] + T[i][1] * A[j, 1]) + T[i][2] * A[j, 2]
                              for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
                o = canon(o)
                if cov == 1:
                    r[:, cov0:cov0 + 24] = o.view(np.uint8).reshape(-1, 24)
                else:
                    r[:, cov0:cov0 + 12] = o.astype(np.float16).view(np.uint8).reshape(-1, 12)
        if sh != 3 and flags & (ROTATE_SH | COLOR):
            c = decode_sh(sh, r[:, sh0:sh0 + SH_BYTES[sh]]).reshape(-1, 15, 3)
            if flags & ROTATE_SH:
                out = c.copy()
                for first, Dm in zip((0, 3, 8), D):
                    Dm = np.asarray(Dm, f32)
                    nbd = Dm.shape[0]
                    for k in range(nbd):
                        acc = Dm[k, 0] * c[:, first, :]
                        for j in range(1, nbd):
                            acc = acc + Dm[k, j] * c[:, first + j, :]
                        out[:, first + k, :] = acc
                c = out
            if flags & COLOR:
                L = np.asarray(color, f32).reshape(4, 3).T[:, :3]
                c = np.stack([lin3(L, c[:, k, :]) for k in range(15)], axis=1)
            r[:, sh0:sh0 + SH_BYTES[sh]] = encode_sh(sh, c.reshape(-1, 45))
        if flags & COLOR:
            Cm = np.asarray(color, f32).reshape(4, 3).T            # 3 x 4
            rgb = r[:, 12:15].astype(f32) / f32(255.0)
            v = lin3(Cm[:, :3], rgb) + Cm[:, 3][None, :]
            r[:, 12:15] = quant_unorm(v)
        if flags & OPACITY:
            a = r[:, 15].astype(f32) / f32(255.0)
            r[:, 15] = quant_unorm(f32(opacity[0]) * a + f32(opacity[1]))
    p = p.copy()
    p[sel] = r
    return p.reshape(-1)
