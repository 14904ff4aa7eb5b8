"""Layout conversion on the device: the converted buffers against the host conversion gs_convert_pods (whose
bytes tests/test_convert_api.py checks against the numpy restatement), the fused compaction against numpy indexing, identical
layouts against extract, the lossy pairs, the concatenation of sources of different layouts, the ordering behind an edit on
another stream, and the frame of a converted buffer against the frame of a direct upload."""
import numpy as np
import pytest

from frames import render_image
from helpers import same_bits
from records import diff, selection_from_mask
from records import rows as _rows
from scenes import ALL_LAYOUTS, packed_pods

pytestmark = pytest.mark.gpu

f32 = np.float32
THREE_PAIRS = [((0, 0), (1, 2)), ((2, 1), (3, 2)), ((1, 2), (0, 1))]


def _ok(src, dst):
    return dst[1] != 0 or src[1] == 0


# ---- bytes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src", ALL_LAYOUTS)
def test_device_bytes_equal_the_host_conversion(gs, device, stream, src):
    n = 5003
    spod = gs.GaussianPod(*src)
    pods = packed_pods(gs, *src, n)
    buf = gs.GaussiansBuffer.new_with_pods(device, spod, pods)
    done = 0
    for dst in ALL_LAYOUTS:
        if not _ok(src, dst):
            continue
        dpod = gs.GaussianPod(*dst)
        out = buf.convert(stream, dpod)
        assert out.pod == dpod and out.len() == n
        got, want = out.download(stream), spod.convert(pods, dpod)
        assert np.array_equal(got, want), (src, dst, diff(got, want, dpod.size))
        out.destroy()
        done += 1
    assert done == (12 if src[1] == 0 else 8)
    assert np.array_equal(buf.download(stream), pods), "the source is untouched"
    buf.destroy()


# ---- compaction ------------------------------------------------------------------------------------------------------

def _masks(n):
    rng = np.random.default_rng(n)
    hole = rng.random(n) < 0.5
    hole[(n // 1024 // 2) * 1024:(n // 1024 // 2 + 1) * 1024] = False      # a whole 1024-block unselected
    hole[-1] = n > 1024                                                    # ... and something behind it
    last = np.zeros(n, bool)
    last[-1] = True
    return [("random", rng.random(n) < 0.3, False), ("empty", np.zeros(n, bool), False), ("all", np.ones(n, bool), False),
            ("hole", hole, False), ("last", last, False), ("invert", rng.random(n) < 0.3, True)]


@pytest.mark.parametrize("n", [1, 63, 1025, 5003])
@pytest.mark.parametrize("src,dst", THREE_PAIRS)
def test_conversion_is_fused_with_the_stable_compaction(gs, device, stream, src, dst, n):
    spod, dpod = gs.GaussianPod(*src), gs.GaussianPod(*dst)
    pods = packed_pods(gs, *src, n)
    buf = gs.GaussiansBuffer.new_with_pods(device, spod, pods)
    for name, mask, invert in _masks(n):
        sel = selection_from_mask(gs, device, stream, mask)
        out = buf.convert(stream, dpod, sel, invert=invert)
        keep = ~mask if invert else mask
        want = spod.convert(np.ascontiguousarray(_rows(pods, spod.size)[keep]).reshape(-1), dpod)
        assert out.len() == int(keep.sum()) and out.pod == dpod, (name, n)          # (convert() itself asserts len == count_out)
        got = out.download(stream)
        assert np.array_equal(got, want), (name, n, diff(got, want, dpod.size))
        if not keep.any():
            assert out.is_empty() and got.size == 0                                 # the valid length-0 buffer
            assert (gs._capi.load().gs_gaussians_buffer_sh(out._h), gs._capi.load().gs_gaussians_buffer_cov3d(out._h)) == dst
        out.destroy(); sel.destroy()
    assert np.array_equal(buf.download(stream), pods)
    buf.destroy()


def test_a_source_of_length_zero(gs, device, stream):
    for src, dst in THREE_PAIRS:
        buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(*src), np.zeros(0, np.uint8))
        for invert in (False, True):
            out = buf.convert(stream, gs.GaussianPod(*dst), None, invert=invert)
            assert out.len() == 0 and out.pod == gs.GaussianPod(*dst) and out.download(stream).size == 0
            out.destroy()
        buf.destroy()


@pytest.mark.parametrize("layout", [(0, 0), (1, 2), (2, 1), (3, 0)])
def test_identical_layouts_equal_extract(gs, device, stream, layout):
    n = 5003
    pod = gs.GaussianPod(*layout)
    pods = np.array(packed_pods(gs, *layout, n))
    # nonzero trailing pad bytes, where the layout has any: identical layouts keep every byte
    used = 16 + [180, 92, 48, 0][layout[0]] + [28, 24, 12][layout[1]]
    _rows(pods, pod.size)[:, used:] = 0xCD
    buf = gs.GaussiansBuffer.new_with_pods(device, pod, pods)
    mask = np.random.default_rng(9).random(n) < 0.3
    sel = selection_from_mask(gs, device, stream, mask)
    for s, inv in ((None, False), (sel, False), (sel, True)):
        a, b = buf.convert(stream, pod, s, invert=inv), buf.extract(stream, s, invert=inv)
        got = a.download(stream)
        assert np.array_equal(got, b.download(stream))
        keep = np.ones(n, bool) if s is None else (~mask if inv else mask)
        assert np.array_equal(_rows(got, pod.size), _rows(pods, pod.size)[keep])
        a.destroy(); b.destroy()
    sel.destroy(); buf.destroy()


# ---- lossy pairs -----------------------------------------------------------------------------------------------------

def test_lossy_pairs_raise_and_create_nothing(gs, device, stream):
    import ctypes as C
    n = 63
    lib = gs._capi.load()
    for src in [(s, c) for s in range(4) for c in (1, 2)]:
        pods = packed_pods(gs, *src, n)
        buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(*src), pods)
        for dsh in range(4):
            with pytest.raises(gs.LossyConfigError):
                buf.convert(stream, gs.GaussianPod(dsh, 0))
            h, count = C.c_void_p(1), C.c_uint64(7)
            rc = lib.gs_gaussians_buffer_create_converted(buf._h, stream._h, None, 0, dsh, 0, C.byref(h), C.byref(count))
            assert rc == gs.LossyConfigError.code and h.value is None and count.value == 0
        assert np.array_equal(buf.download(stream), pods)
        buf.destroy()
    # an unknown config and a selection of another length are argument errors
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(0, 0), packed_pods(gs, 0, 0, n))
    h = C.c_void_p(1)
    assert lib.gs_gaussians_buffer_create_converted(buf._h, stream._h, None, 0, 4, 0, C.byref(h), None) == gs.InvalidArgumentError.code
    assert h.value is None
    short = gs.Selection(device, n - 1)
    with pytest.raises(gs.InvalidArgumentError):
        buf.convert(stream, gs.GaussianPod(1, 2), short)
    short.destroy(); buf.destroy()


# ---- concatenation with a target layout ------------------------------------------------------------------------------

def test_concat_as(gs, device, stream):
    dst = gs.GaussianPod(1, 2)
    layouts, lens = [(0, 0), (1, 2), (3, 1)], [5003, 1025, 2049]
    rows = [packed_pods(gs, *l, n, seed=10 + k) for k, (l, n) in enumerate(zip(layouts, lens))]
    bufs = [gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(*l), r) for l, r in zip(layouts, rows)]
    rng = np.random.default_rng(12)
    order = [0, 1, 2, 0]
    masks = [None, rng.random(1025) < 0.5, None, rng.random(5003) < 0.3]
    sels = [selection_from_mask(gs, device, stream, m) for m in masks]
    out, counts = gs.GaussiansBuffer.concat(stream, [bufs[k] for k in order], sels, pod=dst)
    parts = []
    for k, m in zip(order, masks):
        pod = gs.GaussianPod(*layouts[k])
        r = _rows(rows[k], pod.size)
        parts.append(pod.convert(np.ascontiguousarray(r if m is None else r[m]).reshape(-1), dst))
    assert counts == [len(p) // dst.size for p in parts]
    assert out.pod == dst and out.len() == sum(counts)
    got, want = out.download(stream), np.concatenate(parts)
    assert np.array_equal(got, want), diff(got, want, dst.size)
    for b, r in zip(bufs, rows):
        assert np.array_equal(b.download(stream), r), "the sources are untouched"
    # pod=None is today's call: one layout, bytes unchanged
    plain, c1 = gs.GaussiansBuffer.concat(stream, [bufs[0], bufs[0]], [None, sels[3]])
    same, c2 = gs.GaussiansBuffer.concat(stream, [bufs[0], bufs[0]], [None, sels[3]], pod=None)
    as_same, c3 = gs.GaussiansBuffer.concat(stream, [bufs[0], bufs[0]], [None, sels[3]], pod=gs.GaussianPod(0, 0))
    r0 = _rows(rows[0], 224)
    assert c1 == c2 == c3 == [5003, int(masks[3].sum())] and plain.pod == same.pod == as_same.pod == gs.GaussianPod(0, 0)
    want = np.concatenate([r0, r0[masks[3]]]).reshape(-1)
    for o in (plain, same, as_same):
        assert np.array_equal(o.download(stream), want)
    with pytest.raises(gs.InvalidArgumentError):
        gs.GaussiansBuffer.concat(stream, [bufs[0], bufs[1]])             # two layouts without a target: as before
    # a cov-f16 source with a rot-scale target: nothing is created, nothing is enqueued
    import ctypes as C
    lib = gs._capi.load()
    with pytest.raises(gs.LossyConfigError):
        gs.GaussiansBuffer.concat(stream, [bufs[0], bufs[1]], pod=gs.GaussianPod(1, 0))
    src = (C.c_void_p * 2)(bufs[0]._h, bufs[1]._h)
    h = C.c_void_p(1)
    assert lib.gs_gaussians_buffer_create_concat_as(stream._h, src, None, 2, 1, 0, C.byref(h), None) == gs.LossyConfigError.code
    assert h.value is None
    for b, r in zip(bufs, rows):
        assert np.array_equal(b.download(stream), r)
    for o in [out, plain, same, as_same] + [s for s in sels if s is not None] + bufs:
        o.destroy()


# ---- ordering --------------------------------------------------------------------------------------------------------

def test_convert_is_ordered_behind_an_edit_on_another_stream(gs, device, stream):
    n = 5003
    spod, dpod = gs.GaussianPod(0, 0), gs.GaussianPod(1, 2)
    pods = packed_pods(gs, 0, 0, n)
    s1, s2 = stream, device.create_stream()
    buf = gs.GaussiansBuffer.new_with_pods(device, spod, pods)
    s1.synchronize()
    e = gs.edit(transform=gs.model_transform_pod(pos=(0.5, -0.25, 1.5), rot=(0, 0, 0, 1), scale=(1.25,) * 3), opacity=(0.5, 0.1))
    buf.edit(s1, None, e)
    out = buf.convert(s2, dpod)            # no host synchronisation in between
    s1.synchronize()
    edited = buf.download(s1)
    assert (_rows(edited, 224) != _rows(pods, 224)).any(axis=1).mean() > 0.9
    got, want = out.download(s2), spod.convert(edited, dpod)
    assert np.array_equal(got, want), diff(got, want, dpod.size)
    s2.synchronize()
    out.destroy(); buf.destroy()
    s2.close()


# ---- renderable ------------------------------------------------------------------------------------------------------

def test_a_converted_buffer_renders_like_a_direct_upload(gs, device, stream):
    import synth
    n, W, H = 20000, 256, 256
    g = synth.scene(n, first=31)
    spod, dpod = gs.GaussianPod(0, 0), gs.GaussianPod(1, 2)
    cam = gs.camera_look_at((0, 0, 0), (0, 0, -1), (0, 1, 0), float(np.deg2rad(60.0)), W, H)
    gt, mt = gs.gaussian_transform_pod(sh_deg=3), gs.model_transform_pod()
    src = gs.GaussiansBuffer.new_with_pods(device, spod, spod.from_gaussian(g))
    direct = gs.GaussiansBuffer.new_with_pods(device, dpod, dpod.from_gaussian(g))
    r_src, r_conv, r_direct = gs.Renderer(device), gs.Renderer(device), gs.Renderer(device)
    before, _ = render_image(gs, device, stream, r_src, src, gt, mt, cam, W, H)
    conv = src.convert(stream, dpod)
    assert np.array_equal(conv.download(stream), direct.download(stream))
    assert conv.spatial_order() == src.spatial_order()
    got, fr_c = render_image(gs, device, stream, r_conv, conv, gt, mt, cam, W, H)
    want, fr_d = render_image(gs, device, stream, r_direct, direct, gt, mt, cam, W, H)
    assert fr_d.visible > 1000 and (fr_c.visible, fr_c.pairs) == (fr_d.visible, fr_d.pairs)
    assert np.array_equal(conv.download_order(stream), direct.download_order(stream))
    assert same_bits(got, want)
    after, _ = render_image(gs, device, stream, r_src, src, gt, mt, cam, W, H)
    assert same_bits(after, before), "the source renders as before"
    for o in (r_src, r_conv, r_direct, conv, direct, src):
        o.destroy()
