"""Covariance -> rotation + scale on the device: gs_gaussians_buffer_create_decomposed against the host
function gs_decompose_pods (which tests/test_decompose_api.py checks against a float64 witness) byte for byte — every
covariance layout to every SH config, fused with the compaction, the exact cases at the wave and block edges, behind an edit
on another stream — the frame of a decomposed buffer, the exports with decompose=True against the host path, and the argument
checks."""
import ctypes as C

import numpy as np
import pytest

import decompose_np as dn
from frames import render_image
from helpers import same_bits
from records import diff, selection_from_mask
from records import rows as _rows
from scenes import ALL_LAYOUTS

pytestmark = pytest.mark.gpu

f32 = np.float32
COV_LAYOUTS = [l for l in ALL_LAYOUTS if l[1] != 0]
THREE_PAIRS = [((2, 2), 1), ((0, 1), 3), ((3, 2), 0)]      # (source layout, destination SH); the first: cov f16, snorm8 SH
_PODS = {}


def set_pods(gs, sh, cov, n):
    """the first n Gaussians of the set packed for one layout: once per key, read-only"""
    key = (sh, cov, n)
    if key not in _PODS:
        if "g" not in _PODS:
            _PODS["g"] = dn.set_gaussians(5003, seed=31)
        p = gs.GaussianPod(sh, cov).from_gaussian(_PODS["g"][:n])
        p.setflags(write=False)
        _PODS[key] = p
    return _PODS[key]


# ---- bytes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src", COV_LAYOUTS)
def test_device_bytes_equal_the_host_decomposition(gs, device, stream, src):
    n = 5003
    spod = gs.GaussianPod(*src)
    pods = set_pods(gs, *src, n)
    buf = gs.GaussiansBuffer.new_with_pods(device, spod, pods)
    for dsh in range(4):
        out = buf.decompose(stream, dsh)
        assert out.pod == gs.GaussianPod(dsh, 0) and out.len() == n
        got, want = out.download(stream), spod.decompose(pods, dsh)
        assert np.array_equal(got, want), (src, dsh, diff(got, want, out.pod.size))
        out.destroy()
    keep = buf.decompose(stream)                      # sh=None keeps the SH config
    assert keep.pod == gs.GaussianPod(src[0], 0)
    keep.destroy()
    assert np.array_equal(buf.download(stream), pods), "the source is untouched"
    buf.destroy()


@pytest.mark.parametrize("ssh", range(4))
def test_a_rot_scale_source_is_convert(gs, device, stream, ssh):
    n = 1025
    spod = gs.GaussianPod(ssh, 0)
    buf = gs.GaussiansBuffer.new_with_pods(device, spod, set_pods(gs, ssh, 0, n))
    mask = np.random.default_rng(2).random(n) < 0.3
    sel = selection_from_mask(gs, device, stream, mask)
    for dsh in range(4):
        a, b = buf.decompose(stream, dsh, sel), buf.convert(stream, gs.GaussianPod(dsh, 0), sel)
        assert a.pod == b.pod and np.array_equal(a.download(stream), b.download(stream)), (ssh, dsh)
        a.destroy(); b.destroy()
    sel.destroy(); buf.destroy()


# ---- compaction ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 1025, 5003])
@pytest.mark.parametrize("src,dsh", THREE_PAIRS)
def test_decomposition_is_fused_with_the_stable_compaction(gs, device, stream, src, dsh, n):
    spod, dpod = gs.GaussianPod(*src), gs.GaussianPod(dsh, 0)
    pods = set_pods(gs, *src, n)
    buf = gs.GaussiansBuffer.new_with_pods(device, spod, pods)
    for name, mask, invert in dn.compaction_masks(n):
        sel = selection_from_mask(gs, device, stream, mask)
        out = buf.decompose(stream, dsh, sel, invert=invert)
        keep = ~mask if invert else mask
        want = spod.decompose(np.ascontiguousarray(_rows(pods, spod.size)[keep]).reshape(-1), dsh)
        assert out.len() == int(keep.sum()) and out.pod == dpod, (name, n)
        got = out.download(stream)
        assert np.array_equal(got, want), (name, n, diff(got, want, dpod.size))
        if not keep.any():
            assert out.is_empty() and got.size == 0                                 # the valid length-0 buffer
            lib = gs._capi.load()
            assert (lib.gs_gaussians_buffer_sh(out._h), lib.gs_gaussians_buffer_cov3d(out._h)) == (dsh, 0)
        out.destroy(); sel.destroy()
    assert np.array_equal(buf.download(stream), pods)
    buf.destroy()


# ---- the exact cases at the wave and block edges ---------------------------------------------------------------------

def _special_covariances(gs):
    base = dn.the_set(gs)["f32"]
    out = [f32([4, 0, 0, 0.25, 0, 9]), f32([1e-12, 0, 0, 1e12, 0, 1]), np.zeros(6, f32), f32([-0.0] * 6), f32([3, 0, 0, 3, 0, 3]),
           f32([1e-30, 0, 0, 1e-30, 0, 1e-30])]
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            c = base[k].copy()
            c[k] = bad
            out.append(c)
    for k in (-20, -2, 2, 20):
        out += [base[100] * f32(4.0) ** k, base[-1] * f32(4.0) ** k]
    return out


def test_special_records_at_wave_and_block_edges(gs, device, stream):
    n, places = 2100, (0, 63, 64, 1023, 1024)
    spod = gs.GaussianPod(2, 1)                       # snorm8 SH, cov f32: the covariance words are at byte 64
    specials = _special_covariances(gs)
    for first in range(0, len(specials), len(places)):
        rows = np.array(_rows(set_pods(gs, 2, 1, n), spod.size))
        for at, c in zip(places, specials[first:first + len(places)]):
            rows[at, 64:88] = c.view(np.uint8)
        pods = rows.reshape(-1)
        buf = gs.GaussiansBuffer.new_with_pods(device, spod, pods)
        out = buf.decompose(stream, 2)
        got, want = out.download(stream), spod.decompose(pods, 2)
        assert np.array_equal(got, want), (first, diff(got, want, out.pod.size))
        # the host's records are the exact cases: a non-finite word gives the identity and NaN scales, zero gives zero
        w = _rows(want, out.pod.size)
        for at, c in zip(places, specials[first:first + len(places)]):
            q, s = w[at, 64:80].view(f32), w[at, 80:92].view(f32)
            if not np.isfinite(c).all():
                assert same_bits(q, f32([0, 0, 0, 1])) and (s.view(np.uint32) == 0x7FC00000).all()
            elif not c[[1, 2, 4]].any():      # diagonal, none negative; -0 gives +0 like +0
                assert same_bits(q, f32([0, 0, 0, 1])) and same_bits(s, np.sqrt(np.abs(c[[0, 3, 5]])))
        out.destroy(); buf.destroy()


# ---- ordering --------------------------------------------------------------------------------------------------------

def test_decompose_is_ordered_behind_an_edit_on_another_stream(gs, device, stream):
    n = 5003
    spod = gs.GaussianPod(1, 1)
    pods = set_pods(gs, 1, 1, n)
    s1, s2 = stream, device.create_stream()
    buf = gs.GaussiansBuffer.new_with_pods(device, spod, pods)
    s1.synchronize()
    e = gs.edit(transform=gs.model_transform_pod(pos=(0.5, -0.25, 1.5), rot=(0, 0, 0, 1), scale=(1.25,) * 3), opacity=(0.5, 0.1))
    buf.edit(s1, None, e)
    out = buf.decompose(s2, 1)              # no host synchronisation in between
    s1.synchronize()
    edited = buf.download(s1)
    assert (_rows(edited, spod.size) != _rows(pods, spod.size)).any(axis=1).mean() > 0.9
    got, want = out.download(s2), spod.decompose(edited, 1)
    assert np.array_equal(got, want), diff(got, want, out.pod.size)
    s2.synchronize()
    out.destroy(); buf.destroy()
    s2.close()


# ---- renderable ------------------------------------------------------------------------------------------------------

def test_a_decomposed_buffer_renders_like_a_direct_upload(gs, device, stream):
    import synth
    n, W, H = 3000, 128, 128
    g = synth.scene(n, first=31)
    spod, dpod = gs.GaussianPod(0, 1), gs.GaussianPod(0, 0)
    pods = spod.from_gaussian(g)
    cam = gs.camera_look_at((0, 0, 0), (0, 0, -1), (0, 1, 0), float(np.deg2rad(60.0)), W, H)
    gt, mt = gs.gaussian_transform_pod(sh_deg=3), gs.model_transform_pod()
    src = gs.GaussiansBuffer.new_with_pods(device, spod, pods)
    direct = gs.GaussiansBuffer.new_with_pods(device, dpod, spod.decompose(pods, 0))
    dec = src.decompose(stream)
    assert np.array_equal(dec.download(stream), direct.download(stream))
    assert dec.spatial_order() == src.spatial_order()
    r_dec, r_direct = gs.Renderer(device), gs.Renderer(device)
    got, fr_c = render_image(gs, device, stream, r_dec, dec, gt, mt, cam, W, H)
    want, fr_d = render_image(gs, device, stream, r_direct, direct, gt, mt, cam, W, H)
    assert fr_d.visible > 100 and (fr_c.visible, fr_c.pairs) == (fr_d.visible, fr_d.pairs)
    assert np.array_equal(dec.download_order(stream), direct.download_order(stream))
    assert same_bits(got, want)
    for o in (r_dec, r_direct, dec, direct, src):
        o.destroy()


# ---- save ------------------------------------------------------------------------------------------------------------

def test_save_with_decompose(gs, device, stream, tmp_path):
    n = 5003
    spod = gs.GaussianPod(1, 2)
    pods = set_pods(gs, 1, 2, n)
    buf = gs.GaussiansBuffer.new_with_pods(device, spod, pods)
    mask = np.random.default_rng(4).random(n) < 0.3
    sel = selection_from_mask(gs, device, stream, mask)
    for s, keep in ((None, np.ones(n, bool)), (sel, mask)):
        picked = np.ascontiguousarray(_rows(pods, spod.size)[keep]).reshape(-1)
        g = gs.GaussianPod(1, 0).into_gaussian(spod.decompose(picked, 1))
        assert buf.write(stream, gs.GaussiansSource.Ply, s, decompose=True) == gs.PlyGaussians.from_gaussians(g).write_to()
        assert buf.write(stream, gs.GaussiansSource.Spz, s, decompose=True, fast=True) == \
            gs.gzip_fast(gs.SpzGaussians.write_gaussians_decompressed(g))
        assert buf.write(stream, gs.GaussiansSource.Spz, s, decompose=True) == gs.SpzGaussians.write_gaussians(g)
        assert buf.export_ply(stream, s, decompose=True).pods.tobytes() == gs.gaussian_to_ply(g).tobytes()
        assert buf.export_spz(stream, s, decompose=True).payload == gs.SpzGaussians.write_gaussians_decompressed(g)
    buf.write_to_file(tmp_path / "a.ply", stream, decompose=True)
    g = gs.GaussianPod(1, 0).into_gaussian(spod.decompose(pods, 1))
    assert (tmp_path / "a.ply").read_bytes() == gs.PlyGaussians.from_gaussians(g).write_to()
    # the default is today's behaviour
    for call in (lambda: buf.write(stream, gs.GaussiansSource.Ply), lambda: buf.write(stream, gs.GaussiansSource.Ply, decompose=False),
                 lambda: buf.export_ply(stream), lambda: buf.export_spz(stream), lambda: buf.export_spz_file(stream)):
        with pytest.raises(gs.LossyConfigError):
            call()
    assert np.array_equal(buf.download(stream), pods)
    sel.destroy(); buf.destroy()
    # an SH-less source cannot be exported either way
    nosh = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(3, 2), set_pods(gs, 3, 2, 63))
    for decompose in (False, True):
        with pytest.raises(gs.LossyConfigError):
            nosh.write(stream, gs.GaussiansSource.Ply, decompose=decompose)
        with pytest.raises(gs.LossyConfigError):
            nosh.write(stream, gs.GaussiansSource.Spz, decompose=decompose, fast=True)
    nosh.destroy()


# ---- arguments -------------------------------------------------------------------------------------------------------

def test_argument_errors_create_nothing(gs, device, stream):
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    n = 63
    pods = set_pods(gs, 1, 2, n)
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(1, 2), pods)
    h, count = C.c_void_p(1), C.c_uint64(7)
    assert lib.gs_gaussians_buffer_create_decomposed(None, stream._h, None, 0, 1, C.byref(h), C.byref(count)) == bad and h.value is None
    assert lib.gs_gaussians_buffer_create_decomposed(buf._h, stream._h, None, 0, 1, None, None) == bad
    for dsh in (4, -1):
        h = C.c_void_p(1)
        assert lib.gs_gaussians_buffer_create_decomposed(buf._h, stream._h, None, 0, dsh, C.byref(h), C.byref(count)) == bad
        assert h.value is None and count.value == 0
    short = gs.Selection(device, n - 1)
    h = C.c_void_p(1)
    assert lib.gs_gaussians_buffer_create_decomposed(buf._h, stream._h, short._h, 0, 1, C.byref(h), None) == bad and h.value is None
    with pytest.raises(gs.InvalidArgumentError):
        buf.decompose(stream, 1, short)
    assert np.array_equal(buf.download(stream), pods)
    short.destroy(); buf.destroy()


def test_a_selection_of_another_device_is_refused(gs, device, stream):
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(1, 2), set_pods(gs, 1, 2, 63))
    other = gs.Device(0)          # a second device object: its selections belong to another device
    foreign = gs.Selection(other, 63)
    h = C.c_void_p(1)
    rc = gs._capi.load().gs_gaussians_buffer_create_decomposed(buf._h, stream._h, foreign._h, 0, 1, C.byref(h), None)
    assert rc == gs.InvalidArgumentError.code and h.value is None
    foreign.destroy(); buf.destroy(); other.close()
