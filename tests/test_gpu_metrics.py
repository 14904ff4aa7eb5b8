"""gs_image_compare on the device against the numpy model of tests/metrics_np.py: both planes bit for bit,
counts, maxima and their indices exactly, the binary64 sums inside the first-order bound of a summation, two calls byte for
byte; then the special values (-0, NaN, Inf), one pointer for both images, another data range, the call without SSIM, and
one rendered frame against the frame of its converted buffer."""
import numpy as np
import pytest

import metrics_np

pytestmark = pytest.mark.gpu

f32 = np.float32
_MODEL = {}


def _pair(kind, h, w):
    """the images of a case and the model's result on them, computed once and never written again"""
    key = (kind, h, w)
    if key not in _MODEL:
        a, b = metrics_np.image_pair(kind, h, w)
        want = metrics_np.compare(a, b, ssim=True)
        for v in (a, b) + tuple(x for x in want.values() if isinstance(x, np.ndarray)):
            v.setflags(write=False)
        _MODEL[key] = (a, b, want)
    return _MODEL[key]


class _Device:
    """two images and two planes on the device"""

    def __init__(self, gs, device, a, b, same=False):
        self.gs, self.device = gs, device
        self.h, self.w = a.shape[:2]
        self.a = gs.Buffer(device, data=a)
        self.b = self.a if same else gs.Buffer(device, data=b)
        poison = np.full(self.h * self.w, 0xA5A5A5A5, np.uint32)
        self.err, self.ssim = gs.Buffer(device, data=poison), gs.Buffer(device, data=poison)

    def compare(self, stream, ssim=True, planes=True, data_range=1.0):
        return self.gs.image_compare(self.device, stream, self.a.device_ptr(), self.b.device_ptr(), self.w, self.h, ssim=ssim,
                                     data_range=data_range, err_plane_ptr=self.err.device_ptr() if planes else None,
                                     ssim_plane_ptr=self.ssim.device_ptr() if planes and ssim else None)

    def planes(self, stream):
        return (self.err.download(stream, np.uint32).reshape(self.h, self.w), self.ssim.download(stream, np.uint32).reshape(self.h, self.w))

    def release(self):
        for buf in {id(x): x for x in (self.a, self.b, self.err, self.ssim)}.values():
            buf.release()


def _check_sums(got, want, abs_sum, n, tag):
    """n 2^-52 sum|t|: twice the first-order bound of any summation order in binary64 (the form of tests/test_gpu_stats.py)"""
    bound = np.float64(n) * 2.0 ** -52 * abs_sum
    err = np.abs(got - want)
    print(tag, "err", err, "bound", bound)
    assert (err <= bound).all(), (tag, err, bound)


def _check_record(got, want, tag, ssim=True):
    assert (got.pixels, got.finite, got.differing, got.bit_differing) == (want["pixels"], want["finite"], want["differing"], want["bit_differing"]), tag
    assert got.max_abs.dtype == f32 and got.max_abs_at.dtype == np.uint32
    assert np.array_equal(got.max_abs.view(np.uint32), want["max_abs"].view(np.uint32)), (tag, got.max_abs, want["max_abs"])
    assert np.array_equal(got.max_abs_at, want["max_abs_at"]), (tag, got.max_abs_at, want["max_abs_at"])
    _check_sums(got.sum_sq, want["sum_sq"], want["abs_sq"], want["finite"], tag + ("sum_sq",))
    _check_sums(got.sum_abs, want["sum_abs"], want["abs_abs"], want["finite"], tag + ("sum_abs",))
    if ssim:
        assert np.array_equal(got.ssim_finite, want["ssim_finite"]), (tag, got.ssim_finite, want["ssim_finite"])
        _check_sums(got.ssim_sum, want["ssim_sum"], want["abs_ssim"], want["ssim_finite"].astype(np.float64), tag + ("ssim_sum",))
    else:
        assert not got.ssim_sum.any() and not got.ssim_finite.any(), tag


def _check_planes(dev, stream, want, tag, nan_free=True):
    err, ssim = dev.planes(stream)
    assert np.array_equal(err, want["err_plane"].view(np.uint32)), (tag, "err_plane")
    w = want["ssim_plane"].view(np.uint32)
    if nan_free:
        assert np.array_equal(ssim, w), (tag, "ssim_plane", int((ssim != w).sum()))
    else:       # the sign and payload of a NaN are not part of the definition
        nan = np.isnan(want["ssim_plane"])
        assert np.array_equal(np.isnan(ssim.view(f32)), nan) and np.array_equal(ssim[~nan], w[~nan]), (tag, "ssim_plane")


# ------------------------------------------------------------------------------------------------
# 1. every size and pair against the model
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", metrics_np.PAIRS)
@pytest.mark.parametrize("h,w", metrics_np.SIZES)
def test_compare_equals_the_model(gs, device, stream, h, w, kind):
    a, b, want = _pair(kind, h, w)
    assert np.isfinite(want["ssim_map"]).all()
    dev = _Device(gs, device, a, b)
    got = dev.compare(stream)
    _check_record(got, want, (h, w, kind))
    _check_planes(dev, stream, want, (h, w, kind))
    again = dev.compare(stream)
    assert len(got.raw) == 176 and got.raw == again.raw, "two calls return the same bytes"
    if kind == "equal":
        _, ssim = dev.planes(stream)
        assert (ssim == 0x3F800000).all() and list(got.ssim_sum) == [h * w] * 3 and got.identical and got.ssim == 1.0
        assert got.psnr() == float("inf")
    else:
        assert not got.identical and got.differing > 0
    # without the flag: no SSIM field, the other fields the same bytes; the error plane alone
    plain = dev.compare(stream, ssim=False)
    _check_record(plain, want, (h, w, kind, "plain"), ssim=False)
    assert plain.raw[:128] == got.raw[:128] and plain.raw[128:] == bytes(48)
    err, _ = dev.planes(stream)
    assert np.array_equal(err, want["err_plane"].view(np.uint32))
    bare = dev.compare(stream, planes=False)
    assert bare.raw == got.raw, "the planes do not change the record"
    dev.release()


def test_more_tiles_than_workgroups(gs, device, stream):
    """3 x 65570 pixels are 2050 tiles of 32 x 16: two more than the 2048 workgroups a call starts, so the first two take a
    second tile (and the last tile is two pixels wide)"""
    h, w = 3, 65570
    a, b, want = _pair("noise", h, w)
    dev = _Device(gs, device, a, b)
    got = dev.compare(stream)
    _check_record(got, want, (h, w))
    _check_planes(dev, stream, want, (h, w))
    plain = dev.compare(stream, ssim=False, planes=False)
    assert plain.raw[:128] == got.raw[:128] and plain.raw[128:] == bytes(48)
    assert dev.compare(stream).raw == got.raw
    dev.release()


# ------------------------------------------------------------------------------------------------
# 2. special values
# ------------------------------------------------------------------------------------------------

def test_negative_zero_differs_in_bits_only(gs, device, stream):
    a, _, _ = _pair("noise", 33, 17)
    a, b = a.copy(), a.copy()
    a[20, 9, 1], b[20, 9, 1] = -0.0, 0.0
    dev = _Device(gs, device, a, b)
    got = dev.compare(stream)
    assert got.differing == 0 and got.bit_differing == 1 and not got.identical and got.finite == 33 * 17
    assert not got.sum_sq.any() and not got.max_abs.any() and list(got.max_abs_at) == [0] * 4
    _check_record(got, metrics_np.compare(a, b, ssim=True), ("-0",))
    dev.release()


def test_nan_and_inf_take_out_exactly_their_windows(gs, device, stream):
    h, w = 33, 17
    a, b, _ = _pair("noise", h, w)
    a, b = a.copy(), b.copy()
    a[3, 4, 0] = np.nan          # red of a: the windows of rows 0..8, columns 0..9
    b[25, 12, 2] = np.inf        # blue of b: rows 20..30, columns 7..16
    a[16, 8, 3] = -np.inf        # alpha: no SSIM channel
    want = metrics_np.compare(a, b, ssim=True)
    assert want["finite"] == h * w - 3
    assert list(want["ssim_finite"]) == [h * w - 9 * 10, h * w, h * w - 11 * 10]
    bad = ~np.isfinite(want["ssim_map"])
    assert bad[..., 0].sum() == 90 and bad[:9, :10, 0].all() and bad[20:31, 7:17, 2].all() and not bad[..., 1].any()
    dev = _Device(gs, device, a, b)
    got = dev.compare(stream)
    _check_record(got, want, ("nan",))
    _check_planes(dev, stream, want, ("nan",), nan_free=False)
    err, _ = dev.planes(stream)
    for y, x in ((3, 4), (25, 12), (16, 8)):
        assert err[y, x] == 0x7FC00000
    assert (err != 0x7FC00000).sum() == h * w - 3
    assert dev.compare(stream).raw == got.raw
    dev.release()
    # no finite pixel at all
    none = _Device(gs, device, np.full((5, 7, 4), np.nan, f32), np.zeros((5, 7, 4), f32))
    got = none.compare(stream)
    assert (got.finite, got.differing, got.bit_differing) == (0, 0, 35) and not got.max_abs.any() and list(got.max_abs_at) == [0xFFFFFFFF] * 4
    assert not got.ssim_finite.any() and not got.ssim_sum.any() and not got.sum_sq.any()
    none.release()


def test_one_pointer_for_both_images(gs, device, stream):
    a, _, _ = _pair("out_of_range", 100, 37)
    dev = _Device(gs, device, a, a, same=True)
    got = dev.compare(stream)
    assert got.identical and got.differing == 0 and got.finite == 3700 and list(got.ssim_sum) == [3700.0] * 3
    _check_record(got, metrics_np.compare(a, a, ssim=True), ("same",))
    err, ssim = dev.planes(stream)
    assert not err.any() and (ssim == 0x3F800000).all()
    dev.release()


def test_data_range_255(gs, device, stream):
    a, b, _ = _pair("noise", 100, 37)
    a, b = (a * f32(255.0)).astype(f32), (b * f32(255.0)).astype(f32)
    want = metrics_np.compare(a, b, ssim=True, data_range=255.0)
    dev = _Device(gs, device, a, b)
    got = dev.compare(stream, data_range=255.0)
    _check_record(got, want, ("L=255",))
    _check_planes(dev, stream, want, ("L=255",))
    # the constants matter: with L = 1 the same images give other values
    assert dev.compare(stream, data_range=1.0).ssim_sum[0] != got.ssim_sum[0]
    assert got.psnr(255.0) == pytest.approx(10 * np.log10(255.0 ** 2 / (want["sum_sq"][:3].sum() / (3 * 3700))), rel=1e-12)
    dev.release()


def test_the_library_refuses_bad_arguments_on_a_device(gs, device, stream):
    a, b, _ = _pair("noise", 5, 7)
    dev = _Device(gs, device, a, b)
    p = dev.a.device_ptr()
    with pytest.raises(gs.InvalidArgumentError):
        gs.image_compare(device, stream, p + 4, p, 5, 5)
    with pytest.raises(gs.InvalidArgumentError):
        gs.image_compare(device, stream, p, p, 7, 5, err_plane_ptr=dev.err.device_ptr() + 2)
    dev.release()


# ------------------------------------------------------------------------------------------------
# 3. end to end: a frame of a buffer against the frame of its converted copy
# ------------------------------------------------------------------------------------------------

def test_rendered_frames_of_a_converted_buffer(gs, device, stream):
    import synth
    W, H = 64, 48
    pod = gs.GaussianPodWithShSingleCov3dRotScaleConfigs
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pod.from_gaussian(synth.scene(3000)))
    small = buf.convert(stream, gs.GaussianPod(2, 2))      # SH snorm8, covariance f16
    cam = gs.camera_look_at((0, 0, 0), (0, 0, -1), (0, 1, 0), float(np.deg2rad(60.0)), W, H)
    gt, mt = gs.gaussian_transform_pod(sh_deg=3), gs.model_transform_pod()
    img_a, img_b = gs.Buffer(device, size=W * H * 16), gs.Buffer(device, size=W * H * 16)
    err, ssim = gs.Buffer(device, size=W * H * 4), gs.Buffer(device, size=W * H * 4)
    r = gs.Renderer(device)
    r.render(stream, buf, gt, mt, cam, img_a.device_ptr())
    r.render(stream, small, gt, mt, cam, img_b.device_ptr())
    got = gs.image_compare(device, stream, img_a.device_ptr(), img_b.device_ptr(), W, H, ssim=True, err_plane_ptr=err.device_ptr(),
                           ssim_plane_ptr=ssim.device_ptr())
    a = img_a.download(stream, f32).reshape(H, W, 4)
    b = img_b.download(stream, f32).reshape(H, W, 4)
    want = metrics_np.compare(a, b, ssim=True)
    assert want["finite"] == W * H and 0 < want["differing"], "the conversion changes the picture"
    _check_record(got, want, ("frame",))
    assert np.array_equal(err.download(stream, np.uint32).reshape(H, W), want["err_plane"].view(np.uint32))
    assert np.array_equal(ssim.download(stream, np.uint32).reshape(H, W), want["ssim_plane"].view(np.uint32))
    print("frame: psnr %.2f dB  ssim %.5f  max %s" % (got.psnr(), got.ssim, got.max_abs))
    assert 20.0 < got.psnr() < float("inf") and 0.5 < got.ssim < 1.0      # a quantised copy, not another scene
    r.destroy()
    for x in (img_a, img_b, err, ssim):
        x.release()
