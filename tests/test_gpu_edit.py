"""Edits of the selected Gaussians on the device and their extraction: the edited bytes against the numpy
binary32 restatement of tests/edit_np.py, the quantised SH layouts against the f32 layout, the frames after an edit
against a fresh upload and the oracle, a baked transform against the same model transform, the stable compaction against
numpy indexing, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import edit_np
import helpers
import records
import scenes
from frames import render_image

pytestmark = pytest.mark.gpu

f32 = np.float32


# ------------------------------------------------------------------------------------------------
# 1. byte equality with the restatement
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh,cov", scenes.ALL_LAYOUTS)
def test_edit_bytes_equal_the_restatement(gs, device, stream, sh, cov):
    n = 5003
    pod = gs.GaussianPod(sh, cov)
    assert pod.size == edit_np.pod_bytes(sh, cov)
    pods = pod.from_gaussian(scenes.hostile_scene(n))
    mask = np.random.default_rng(1).random(n) < 0.3
    sel = gs.Selection(device, n)
    sel.upload(stream, mask)
    T, R, Cf, O = gs.EDIT_TRANSFORM, gs.EDIT_ROTATE_SH, gs.EDIT_COLOR, gs.EDIT_OPACITY
    cases = [(T | R | Cf | O, mask), (T, mask), (T | R, mask), (Cf, mask), (O, mask), (T | R | Cf | O, None), (Cf | O, None)]
    for flags, m in cases:
        buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
        buf.edit(stream, sel if m is not None else None, records.sample_edit(gs, flags))
        got = buf.download(stream)
        want = records.edited_pods(gs, sh, cov, pods, m, flags)
        assert np.array_equal(got, want), (flags, m is not None, records.diff(got, want, pod.size))
        if m is not None:       # outside the selection every byte stays
            assert np.array_equal(got.reshape(n, -1)[~m], np.asarray(pods).reshape(n, -1)[~m])
        changed = (got.reshape(n, -1) != np.asarray(pods).reshape(n, -1)).any(axis=0)
        if flags == O:
            assert changed[15] and not np.delete(changed, 15).any()
        if flags == T and sh != 3:
            assert not changed[12:16 + edit_np.SH_BYTES[sh]].any()
        if flags == Cf:
            assert not changed[:12].any() and not changed[15] and not changed[16 + edit_np.SH_BYTES[sh]:].any()
        buf.destroy()
    # flags == 0: nothing happens; ROTATE_SH on an SH-less layout is ignored
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    buf.edit(stream, None, gs.edit())
    assert np.array_equal(buf.download(stream), pods)
    buf.destroy(); sel.destroy()


# ------------------------------------------------------------------------------------------------
# 2. quantised SH layouts
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh", [1, 2])
def test_rotated_sh_on_quantised_layouts(gs, device, stream, sh):
    """The f16 / snorm8 layout and the f32 layout start from the SAME coefficient values (the quantised layout's, decoded),
    so the edit computes the same binary32 result v on both and the quantised layout stores its encoding of v: round to
    nearest even for f16 — at most half an ulp, 2^-11 relative (2^-25 absolute below the normal range), inside the one
    step 2^-10 allowed; truncation of clamp(v 127, -127, 127) for snorm8 — less than one step 1 / 127, which is checked
    on the stored bytes in units of the step (|b - 127 clamp(v, -1, 1)| <= 1, exact in float64) so that the decode's own
    division does not enter."""
    n = 4000
    g = scenes.hostile_scene(n)
    g["sh"] = np.random.default_rng(4).uniform(-1, 1, (n, 45)).astype(f32)
    podq, pod32 = gs.GaussianPod(sh, 0), gs.GaussianPod(0, 0)
    pq = podq.from_gaussian(g)
    dec = edit_np.decode_sh(sh, np.asarray(pq).reshape(n, -1)[:, 16:16 + edit_np.SH_BYTES[sh]])
    g["sh"] = dec
    p32 = pod32.from_gaussian(g)
    e = records.sample_edit(gs, gs.EDIT_TRANSFORM | gs.EDIT_ROTATE_SH)
    out = []
    for pod, p in ((podq, pq), (pod32, p32)):
        buf = gs.GaussiansBuffer.new_with_pods(device, pod, p)
        buf.edit(stream, None, e)
        out.append(np.asarray(buf.download(stream)).reshape(n, -1))
        buf.destroy()
    vq = edit_np.decode_sh(sh, out[0][:, 16:16 + edit_np.SH_BYTES[sh]]).astype(np.float64)
    v = edit_np.decode_sh(0, out[1][:, 16:196]).astype(np.float64)
    assert np.abs(v - dec).max() > 0.1, "the rotation must change the coefficients"
    if sh == 1:
        err, tol = np.abs(vq - v), np.maximum(2.0 ** -10 * np.abs(v), 2.0 ** -24)
    else:
        b = np.ascontiguousarray(out[0][:, 16:16 + 45]).view(np.int8).astype(np.float64)
        assert np.array_equal(np.maximum(b / 127.0, -1.0).astype(f32), vq.astype(f32))
        err, tol = np.abs(b - 127.0 * np.clip(v, -1, 1)) / 127.0, 1.0 / 127
    print("sh layout %d: max error %.3g" % (sh, err.max()), "max error / tolerance %.3g" % (err / tol).max())
    assert (err <= tol).all()


# ------------------------------------------------------------------------------------------------
# 3. frames after an edit
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spatial", [False, True])
@pytest.mark.parametrize("flags", [15, 12])       # everything; colour + opacity (the mirror keeps its order)
def test_frames_after_an_edit(gs, ob, device, stream, spatial, flags):
    import synth
    n, W, H, sh, cov = 1500, 320, 192, 0, 0
    g = synth.scene(n, first=21)
    pod = gs.GaussianPod(sh, cov)
    pods = pod.from_gaussian(g)
    mask = np.random.default_rng(2).random(n) < 0.3
    ogt, omt = ob.gaussian_transform(sh_deg=3), ob.model_transform()
    ocam = helpers.default_camera(ob, W, H)
    gt, mt = gs.GaussianTransformPod.from_buffer_copy(bytes(ogt)), gs.ModelTransformPod.from_buffer_copy(bytes(omt))
    cam = helpers.copy_camera(ocam, gs.Camera)
    if spatial:
        # the mirror order is observable only where two Gaussians have bit-identical view depths (§3.4a): none here
        proj, tiles = ob.preprocess(sh, cov, records.edited_pods(gs, sh, cov, pods, mask, flags), ogt, omt, ocam)
        depth = proj["depth"][np.asarray(tiles) > 0]
        assert len(depth) > 100 and len(np.unique(depth.view(np.uint32))) == len(depth)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    buf.set_spatial_order(spatial)
    sel = gs.Selection(device, n)
    sel.upload(stream, mask)
    r1, r2 = gs.Renderer(device), gs.Renderer(device)
    stream2 = device.create_stream()
    before, _ = render_image(gs, device, stream, r1, buf, gt, mt, cam, W, H)         # r1 has rendered the buffer; the mirror is current
    buf.edit(stream, sel, records.sample_edit(gs, flags))
    # a second renderer on ANOTHER stream right behind the edit, with no host synchronisation in between
    after2, _ = render_image(gs, device, stream2, r2, buf, gt, mt, cam, W, H)
    after1, fr1 = render_image(gs, device, stream, r1, buf, gt, mt, cam, W, H)
    edited = buf.download(stream)
    assert np.array_equal(edited, records.edited_pods(gs, sh, cov, pods, mask, flags))
    fresh = gs.GaussiansBuffer.new_with_pods(device, pod, edited)
    fresh.set_spatial_order(spatial)
    r3 = gs.Renderer(device)
    want, fr3 = render_image(gs, device, stream, r3, fresh, gt, mt, cam, W, H)
    assert not helpers.same_bits(before, want), "the edit must change the frame"
    assert helpers.same_bits(after1, want) and helpers.same_bits(after2, want)
    assert (fr1.visible, fr1.pairs) == (fr3.visible, fr3.pairs)
    assert np.array_equal(buf.download_order(stream), fresh.download_order(stream))
    ref, d, vis, _ = ob.render(sh, cov, edited, ogt, omt, ocam, order=fresh.download_order(stream))
    assert helpers.same_bits(want, ref) and (fr3.visible, fr3.pairs) == (vis, d)
    stream2.synchronize(); stream2.close()
    for o in (r1, r2, r3, sel, buf, fresh):
        o.destroy()


# ------------------------------------------------------------------------------------------------
# 4. a baked transform renders like the same model transform
# ------------------------------------------------------------------------------------------------

def _rot64(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _basis64(d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy = x * x, y * y, z * z, x * y
    return np.stack([-0.4886025119029199 * y, 0.4886025119029199 * z, -0.4886025119029199 * x,
                     1.0925484305920792 * xy, -1.0925484305920792 * y * z, 0.31539156525252005 * (2 * zz - xx - yy),
                     -1.0925484305920792 * x * z, 0.5462742152960396 * (xx - yy),
                     -0.5900435899266435 * y * (3 * xx - yy), 2.890611442640554 * xy * z,
                     -0.4570457994644658 * y * (4 * zz - xx - yy), 0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy),
                     -0.4570457994644658 * x * (4 * zz - xx - yy), 1.445305721320277 * z * (xx - yy),
                     -0.5900435899266435 * x * (xx - 3 * yy)], axis=1)


def _bake64(g, q, pos, s, rotate_sh=True):
    """the transform baked into the Gaussians in float64 numpy: position, rotation, scale and the SH rest coefficients
    (D from a least-squares solve of the defining property over random directions)"""
    R = _rot64(q)
    out = g.copy()
    out["pos"] = (s * (g["pos"].astype(np.float64) @ R.T) + np.asarray(pos, np.float64)).astype(f32)
    r = g["rot"].astype(np.float64)
    qx, qy, qz, qw = [float(v) for v in q]
    rx, ry, rz, rw = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    out["rot"] = np.stack([qw * rx + qx * rw + qy * rz - qz * ry, qw * ry - qx * rz + qy * rw + qz * rx,
                           qw * rz + qx * ry - qy * rx + qz * rw, qw * rw - qx * rx - qy * ry - qz * rz], axis=1).astype(f32)
    out["scale"] = (s * g["scale"].astype(np.float64)).astype(f32)
    if rotate_sh:
        d = np.random.default_rng(0).normal(size=(400, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        D = np.linalg.lstsq(_basis64(d), _basis64(d @ R), rcond=None)[0]        # Y(d)^T D = Y(R^T d)^T
        c = g["sh"].astype(np.float64).reshape(-1, 15, 3)
        out["sh"] = np.einsum("kj,njc->nkc", D, c).reshape(-1, 45).astype(f32)
    return out


def _bake_scene(n):
    import synth
    g = synth.scene(n, first=33)
    rng = np.random.default_rng(33)
    g["color"][:, 3] = rng.integers(60, 140, n)          # moderate opacity
    g["scale"] = np.maximum(g["scale"], f32(0.05)) * f32(5.0)    # smooth splats: no sub-pixel needles
    g["sh"] = rng.uniform(-0.6, 0.6, (n, 45)).astype(f32)        # a strong view dependence
    return g


@pytest.mark.parametrize("cov", [0, 1])
def test_bake_equals_model_transform(gs, ob, device, stream, cov):
    """render(buffer, model_transform = T) against render(edit(buffer, T), identity).  The two differ by rounding and by the
    frame's discontinuous decisions (cull, tile rect, skip / stop), so the allowance is measured at run time on the CPU
    oracle: twice the per-pixel maximum of the same pair there (baked side in float64 numpy) plus the contract's 1e-4; at
    most 0.1 % of the pixels may exceed it.  Oracle pair, measured on the CPU: max 3.58e-6 for both layouts (allowance
    1.07e-4); the oracle's frame of the binary32-baked records (tests/edit_np.py) differs from the model-transform frame
    by 3.6e-7 at most; without ROTATE_SH the pair differs by up to 0.64, beyond the allowance on 54 % of the pixels."""
    n, W, H, sh = 4000, 320, 192, 0
    g = _bake_scene(n)
    q, pos, s = records.Q, (0.3, -0.2, -0.4), 1.2
    pod = gs.GaussianPod(sh, cov)
    ogt, oid = ob.gaussian_transform(sh_deg=3), ob.model_transform()
    omt = ob.model_transform(pos=pos, rot=q, scale=(s, s, s))
    ocam = helpers.default_camera(ob, W, H)
    gt = gs.GaussianTransformPod.from_buffer_copy(bytes(ogt))
    ident, mt = gs.ModelTransformPod.from_buffer_copy(bytes(oid)), gs.ModelTransformPod.from_buffer_copy(bytes(omt))
    cam = helpers.copy_camera(ocam, gs.Camera)
    pods = pod.from_gaussian(g)
    # the oracle pair
    o_model = ob.render(sh, cov, pods, ogt, omt, ocam)[0]
    o_baked = ob.render(sh, cov, ob.pack(sh, cov, _bake64(g, q, pos, s)), ogt, oid, ocam)[0]
    o_max = float(np.abs(o_model - o_baked).max())
    allow = 2.0 * o_max + 1e-4
    print("cov %d: oracle pair max %.3g, allowance %.3g" % (cov, o_max, allow))
    assert o_max < 1e-2, "the scene must keep the oracle pair away from the frame's discontinuities"
    assert o_model[..., 3].mean() > 0.2, "the scene must cover the image"
    # the GPU pair
    r = gs.Renderer(device)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    a, _ = render_image(gs, device, stream, r, buf, gt, mt, cam, W, H)
    e = gs.edit(transform=gs.model_transform_pod(pos=pos, rot=q, scale=(s, s, s)))
    assert e.flags == gs.EDIT_TRANSFORM | gs.EDIT_ROTATE_SH
    buf.edit(stream, None, e)
    b, _ = render_image(gs, device, stream, r, buf, gt, ident, cam, W, H)
    diff = np.abs(a - b).max(axis=2)
    over = float((diff > allow).mean())
    print("gpu pair max %.3g, pixels beyond the allowance %.4f %%" % (float(diff.max()), 100 * over))
    assert over <= 1e-3
    # without the SH rotation the view dependence points the wrong way: far beyond the allowance
    buf2 = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    buf2.edit(stream, None, gs.edit(transform=gs.model_transform_pod(pos=pos, rot=q, scale=(s, s, s)), rotate_sh=False))
    c, _ = render_image(gs, device, stream, r, buf2, gt, ident, cam, W, H)
    diff2 = np.abs(a - c).max(axis=2)
    print("without ROTATE_SH: max %.3g, pixels beyond the allowance %.2f %%" % (float(diff2.max()), 100 * float((diff2 > allow).mean())))
    assert (diff2 > allow).mean() > 1e-3
    for o in (r, buf, buf2):
        o.destroy()


# ------------------------------------------------------------------------------------------------
# 5. extraction
# ------------------------------------------------------------------------------------------------

def _check_extract(gs, device, stream, sh, cov, n, seed):
    pod = gs.GaussianPod(sh, cov)
    rng = np.random.default_rng(seed)
    pods = rng.integers(0, 256, n * pod.size, dtype=np.uint8)        # a byte copy: any bytes do
    rows = pods.reshape(n, -1)
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    sel = gs.Selection(device, n)
    masks = [rng.random(n) < 0.3, rng.random(n) < 0.97, np.zeros(n, bool), np.ones(n, bool)]
    if n > 2048:
        m = np.zeros(n, bool)
        m[1024:2048] = True             # one whole block
        m[n - 1] = True
        masks.append(m)
    for mask in masks:
        sel.upload(stream, mask)
        for invert in (False, True):
            want = rows[~mask] if invert else rows[mask]
            out = buf.extract(stream, sel, invert=invert)
            assert out.len() == len(want) and out.pod == pod
            count = C.c_uint64(12345)
            h = C.c_void_p()
            gs._check(gs._L.gs_gaussians_buffer_create_from_selection(buf._h, stream._h, sel._h, int(invert), C.byref(h), C.byref(count)))
            assert count.value == len(want)
            gs._L.gs_gaussians_buffer_destroy(h)
            assert np.array_equal(out.download(stream), want.reshape(-1)), (n, int(mask.sum()), invert)
            out.destroy()
    # no selection: everything, or nothing
    out = buf.extract(stream, None)
    assert np.array_equal(out.download(stream), pods)
    out.destroy()
    out = buf.extract(stream, None, invert=True)
    assert out.len() == 0 and out.is_empty() and out.download(stream).size == 0
    out.destroy()
    assert np.array_equal(buf.download(stream), pods), "the source is untouched"
    short = gs.Selection(device, n + 1)
    with pytest.raises(gs.InvalidArgumentError):
        buf.extract(stream, short)
    short.destroy(); sel.destroy(); buf.destroy()


@pytest.mark.parametrize("n", [1, 33, 1024, 100003])
def test_extract_sizes(gs, device, stream, n):
    _check_extract(gs, device, stream, 0, 0, n, n)


@pytest.mark.parametrize("sh,cov", scenes.ALL_LAYOUTS)
def test_extract_all_layouts(gs, device, stream, sh, cov):
    _check_extract(gs, device, stream, sh, cov, 5003, sh * 3 + cov)


def test_delete_equals_hide(gs, device, stream):
    """the frame of extract(S, invert = True) is, bit for bit, the hide = S frame of the source (index order: the stable
    compaction keeps the order of exact-depth ties)"""
    import synth
    n, W, H = 30_001, 333, 197
    pod = gs.GaussianPod(0, 0)
    pods = pod.from_gaussian(synth.scene(n, first=7))
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    buf.set_spatial_order(False)
    mask = np.random.default_rng(9).random(n) < 0.4
    sel = gs.Selection(device, n)
    sel.upload(stream, mask)
    gt, mt = gs.gaussian_transform_pod(sh_deg=3), gs.model_transform_pod()
    cam = gs.camera_look_at((0, 0, 0), (0, 0, -1), (0, 1, 0), float(np.deg2rad(60.0)), W, H)
    r1, r2 = gs.Renderer(device), gs.Renderer(device)
    hidden, fh = render_image(gs, device, stream, r1, buf, gt, mt, cam, W, H, hide=sel)
    kept = buf.extract(stream, sel, invert=True)
    assert not kept.spatial_order() and kept.len() == int((~mask).sum())
    deleted, fd = render_image(gs, device, stream, r2, kept, gt, mt, cam, W, H)
    assert helpers.same_bits(hidden, deleted) and (fh.visible, fh.pairs) == (fd.visible, fd.pairs) and fh.visible > 0
    for o in (r1, r2, sel, kept, buf):
        o.destroy()


# ------------------------------------------------------------------------------------------------
# 6. argument errors leave the buffer as it is
# ------------------------------------------------------------------------------------------------

def test_argument_errors_leave_the_bytes(gs, device, stream):
    n = 777
    pod = gs.GaussianPod(0, 0)
    pods = pod.from_gaussian(scenes.hostile_scene(n))
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    sel = gs.Selection(device, n)
    sel.fill(stream)
    short = gs.Selection(device, n - 1)
    good = records.sample_edit(gs, 15)

    def variant(**kw):
        e = gs.Edit.from_buffer_copy(bytes(good))
        for k, v in kw.items():
            if k == "flags":
                e.flags = v
            elif k == "reserved":
                e.reserved[2] = v
            else:
                obj, idx = k.split("_")
                getattr(e.transform if obj in ("pos", "rot", "scale") else e, obj)[int(idx)] = v
        return e
    bad = [variant(flags=16), variant(flags=15 | 1 << 31), variant(reserved=1), variant(flags=gs.EDIT_ROTATE_SH),
           variant(flags=gs.EDIT_ROTATE_SH | gs.EDIT_COLOR),
           variant(pos_1=np.nan), variant(rot_0=np.inf), variant(scale_0=np.nan), variant(color_7=np.nan), variant(opacity_1=-np.inf),
           variant(scale_1=2.0), variant(scale_0=-1.25, scale_1=-1.25, scale_2=-1.25), variant(scale_0=0.0, scale_1=0.0, scale_2=0.0),
           variant(rot_0=0.0, rot_1=0.0, rot_2=0.0, rot_3=0.0)]
    for e in bad:
        with pytest.raises(gs.InvalidArgumentError):
            buf.edit(stream, sel, e)
    with pytest.raises(gs.InvalidArgumentError):
        buf.edit(stream, short, good)
    assert gs._L.gs_gaussians_buffer_edit(buf._h, stream._h, sel._h, None) == gs.InvalidArgumentError.code
    assert gs._L.gs_gaussians_buffer_edit(None, stream._h, sel._h, C.byref(good)) == gs.InvalidArgumentError.code
    stream.synchronize()
    assert np.array_equal(buf.download(stream), pods)
    # a field that the flags do not use may hold anything
    e = variant(flags=gs.EDIT_OPACITY, pos_0=np.nan, color_0=np.inf, scale_1=7.0)
    buf.edit(stream, sel, e)
    assert np.array_equal(buf.download(stream), records.edited_pods(gs, 0, 0, pods, None, gs.EDIT_OPACITY))
    short.destroy(); sel.destroy(); buf.destroy()
