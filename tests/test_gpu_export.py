"""Export on the device: gs_gaussians_buffer_export_ply / _export_spz_decompressed / _export_spz / _write against
the host path of the same library — extract, download_gaussians, then gs_gaussian_to_ply / gs_spz_encode_decompressed — byte for
byte, at the wave (64), workgroup (128, 256) and 1024-block edges, for every selection shape and the three layouts that can be
exported; against tests/golden/export_v1.npz (the oracle's bytes, recorded on glibc 2.35); through a PLY file and back; the
refused layouts, a short capacity, and the ordering behind an edit on another stream."""
import ctypes as C
import os

import numpy as np
import pytest

import gpu_child
from records import first_difference, selection_from_mask
from scenes import export_scene, export_selections, golden_export

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000]
EXPORTABLE = [(0, 0), (1, 0), (2, 0)]
REFUSED = [(s, c) for s in range(4) for c in range(3) if (s, c) not in EXPORTABLE]
SPZ_CONFIGS = [(v, d, b) for v in (1, 2, 3) for d in (0, 3) for b in (8, 4)]
INVALID_ARGUMENT = -1


def _spz_options(gs, cfg):
    v, d, b = cfg
    return gs.spz_options(version=v, sh_degree=d, sh_quantize_bits=(b, b, b))


# ---- PLY -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", EXPORTABLE)
def test_export_ply_equals_the_host_path(gs, device, stream, layout):
    pod = gs.GaussianPod(*layout)
    done = 0
    for n in SIZES:
        buf = gs.GaussiansBuffer.new(device, pod, export_scene(n))
        for name, mask, invert in export_selections(n):
            sel = selection_from_mask(gs, device, stream, mask)
            picked = buf.extract(stream, sel, invert)
            want = gs.gaussian_to_ply(picked.download_gaussians(stream))
            got = buf.export_ply(stream, sel, invert)
            keep = np.ones(n, bool) if mask is None else (~mask if invert else mask)
            assert len(got) == len(want) == int(keep.sum()), (n, name)
            assert np.array_equal(got.pods.view(np.uint32), want.view(np.uint32)), (n, name, first_difference(got.pods.tobytes(), want.tobytes(), 248))
            picked.destroy()
            if sel is not None:
                sel.destroy()
            done += 1
        buf.destroy()
    assert done == len(SIZES) * 8


def test_export_ply_decodes_the_records_of_the_buffer(gs, device, stream):
    """... and the host path itself starts from the records the caller uploaded: to_ply of the scene, selected with numpy"""
    n = 3000
    g = export_scene(n)
    buf = gs.GaussiansBuffer.new(device, gs.GaussianPod(0, 0), g)
    mask = np.random.default_rng(5).random(n) < 0.3
    sel = selection_from_mask(gs, device, stream, mask)
    assert buf.export_ply(stream, sel).pods.tobytes() == gs.gaussian_to_ply(g[mask]).tobytes()
    assert buf.export_ply(stream, sel, invert=True).pods.tobytes() == gs.gaussian_to_ply(g[~mask]).tobytes()
    sel.destroy(); buf.destroy()


_SLICE_CHILD = r"""
import sys
sys.path.insert(0, %r)
import importlib.util, os, numpy as np
import wgpu_3dgs_core_amd as gs
spec = importlib.util.spec_from_file_location("mk", os.path.join(%r, "tests", "golden", "make_golden_export.py"))
mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)
n = 3000
g = mk.scene(n)
dev = gs.Device(0)
st = dev.create_stream()
rng = np.random.default_rng(9)
hole = rng.random(n) < 0.3
hole[1024:2048] = False                 # a slice that selects nothing
for layout in ((0, 0), (2, 0)):
    buf = gs.GaussiansBuffer.new(dev, gs.GaussianPod(*layout), g)
    src = buf.download_gaussians(st)
    for mask in (None, rng.random(n) < 0.3, hole):
        sel = None
        if mask is not None:
            sel = gs.Selection(dev, n); sel.upload(st, mask)
        want = gs.gaussian_to_ply(src if mask is None else src[mask])
        got = buf.export_ply(st, sel)
        assert got.pods.tobytes() == want.tobytes(), (layout, "ply")
        image = buf.write(st, gs.GaussiansSource.Ply, sel)
        assert image == gs.PlyGaussians(want).write_to(), (layout, "file image")
print("slices OK")
"""


def test_export_ply_across_slice_boundaries():
    """n = 3000 with GS3D_EXPORT_SLICE=1024: three slices, two boundaries, both staging buffers (the switch is read once per
    process, hence the child)"""
    gpu_child.run(["-c", _SLICE_CHILD % (ROOT, ROOT)], env={"GS3D_EXPORT_SLICE": "1024"}, timeout=120,
                  label="GS3D_EXPORT_SLICE=1024", expect="slices OK")


# ---- SPZ -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", EXPORTABLE)
def test_export_spz_equals_the_host_encoder(gs, device, stream, layout):
    pod = gs.GaussianPod(*layout)
    for n in SIZES:
        buf = gs.GaussiansBuffer.new(device, pod, export_scene(n))
        src = buf.download_gaussians(stream)
        for name, mask, invert in export_selections(n):
            sel = selection_from_mask(gs, device, stream, mask)
            picked = src if mask is None else src[~mask if invert else mask]
            for cfg in SPZ_CONFIGS:
                opt = _spz_options(gs, cfg)
                want = gs.SpzGaussians.write_gaussians_decompressed(picked, opt)
                got = buf.export_spz(stream, sel, invert, opt)
                assert len(got) == len(picked)
                assert got.payload == want, (n, name, cfg, first_difference(got.payload, want, 1))
            if sel is not None:
                sel.destroy()
        buf.destroy()


def test_export_spz_default_options_and_gzip_member(gs, device, stream):
    n = 1025
    buf = gs.GaussiansBuffer.new(device, gs.GaussianPod(0, 0), export_scene(n))
    src = buf.download_gaussians(stream)
    mask = np.arange(n) % 3 != 0
    sel = selection_from_mask(gs, device, stream, mask)
    assert buf.export_spz(stream, sel).payload == gs.SpzGaussians.write_gaussians_decompressed(src[mask])
    assert buf.write(stream, gs.GaussiansSource.Spz, sel) == gs.SpzGaussians.write_gaussians(src[mask])
    assert buf.write(stream, gs.GaussiansSource.Spz) == gs.Gaussians.from_gaussians_iter(src, gs.GaussiansSource.Spz).write_to()
    with pytest.raises(gs.GsError):
        buf.export_spz(stream, sel, options=gs.spz_options(version=4))
    with pytest.raises(gs.InvalidArgumentError):
        buf.export_spz(stream, sel, options=gs.spz_options(sh_quantize_bits=(9, 9, 9)))
    sel.destroy(); buf.destroy()


def test_write_to_file_picks_the_format_by_suffix(gs, device, stream, tmp_path):
    n = 257
    buf = gs.GaussiansBuffer.new(device, gs.GaussianPod(1, 0), export_scene(n))
    src = buf.download_gaussians(stream)
    buf.write_to_file(str(tmp_path / "a.ply"), stream)
    buf.write_to_file(str(tmp_path / "a.spz"), stream)
    assert (tmp_path / "a.ply").read_bytes() == gs.PlyGaussians.from_gaussians(src).write_to()
    assert (tmp_path / "a.spz").read_bytes() == gs.SpzGaussians.write_gaussians(src)
    buf.destroy()


# ---- golden ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [(0, 0)])
def test_device_export_equals_the_golden_bytes(gs, device, stream, layout):
    """the 300 records of export_v1.npz, uploaded as f32 / rot-scale (which keeps every bit of them) and exported: the
    oracle's bytes, whatever the C library of this machine"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "export_v1.npz"))
    g = np.ascontiguousarray(gold["gaussians"]).view(gs.GAUSSIAN_DTYPE).reshape(-1)
    buf = gs.GaussiansBuffer.new(device, gs.GaussianPod(*layout), g)
    assert buf.export_ply(stream).pods.tobytes() == gold["ply"].tobytes()
    for cfg in golden_export().GOLDEN_CONFIGS:
        assert buf.export_spz(stream, options=_spz_options(gs, cfg)).payload == gold["spz_v%d_d%d_b%d" % cfg].tobytes(), cfg
    buf.destroy()


# ---- round trip ------------------------------------------------------------------------------------------------------

def _round_trip_scene(gs, n):
    """Finite records whose quaternion Gaussian::from_ply's normalisation leaves unchanged.  from_ply divides the quaternion
    by its computed length, and for a quaternion that was normalised ONCE that length is not always exactly 1: 1023 of 3000
    such quaternions move by an ulp when they are read back (measured on the host encoders, which are the device's).  That is
    the reference's arithmetic, not the exporter's, so the scene holds fixed points of the normalisation and the rotation check
    below is exact: the quaternions are normalised a few more times, and the few that keep moving between two neighbours
    (16 of 1500) take the quaternion of a record that has settled."""
    rng = np.random.default_rng(23)
    g = np.array(golden_export().scene(n + 2000)[1100:1100 + n])          # a stretch without hostile records
    assert np.isfinite(g["scale"]).all() and (g["scale"] > 0).all() and np.isfinite(g["rot"]).all()
    g["color"][:, 3] = rng.integers(0, 256, n)
    g["color"][:4, 3] = (0, 255, 1, 254)
    for _ in range(6):
        g["rot"] = gs.gaussian_from_ply(gs.gaussian_to_ply(g))["rot"]
    back = gs.gaussian_from_ply(gs.gaussian_to_ply(g))
    moving = (back["rot"].view(np.uint32) != g["rot"].view(np.uint32)).any(axis=1)
    assert 0 < (~moving).sum() and moving.sum() < n // 10
    g["rot"][moving] = g["rot"][~moving][:moving.sum()]
    back = gs.gaussian_from_ply(gs.gaussian_to_ply(g))
    assert np.array_equal(back["rot"].view(np.uint32), g["rot"].view(np.uint32))
    assert len(np.unique(g["rot"].view(np.uint32), axis=0)) > n * 0.9
    return g


def test_ply_file_round_trip(gs, device, stream):
    n = 1500
    pod = gs.GaussianPod(0, 0)
    g = _round_trip_scene(gs, n)
    buf = gs.GaussiansBuffer.new(device, pod, g)
    before = buf.download(stream).view(np.uint32).reshape(n, 56)
    image = buf.write(stream, gs.GaussiansSource.Ply)
    ply = gs.PlyGaussians.read_from(image)
    assert ply.inria and len(ply) == n
    again = gs.GaussiansBuffer.new_from_ply(device, pod, ply)
    after = again.download(stream).view(np.uint32).reshape(n, 56)
    # f32 / rot-scale records: pos @0, colour @3, sh @4, rot @49, scale @53
    assert np.array_equal(after[:, 0:3], before[:, 0:3]), "position bits"
    assert np.array_equal(after[:, 4:49], before[:, 4:49]), "SH bits"
    assert np.array_equal(after[:, 49:53], before[:, 49:53]), "rotation bits"
    ca, cb = after[:, 3:4].copy().view(np.uint8).astype(int), before[:, 3:4].copy().view(np.uint8).astype(int)
    print("colour bytes: largest difference %d" % np.abs(ca - cb).max())
    assert np.abs(ca - cb).max() <= 1
    sa, sb = after[:, 53:56].copy().view(np.float32).astype(np.float64), before[:, 53:56].copy().view(np.float32).astype(np.float64)
    rel = np.abs(sa - sb) / np.abs(sb)
    print("scale: largest relative difference %.3g" % rel.max())
    assert rel.max() <= 1e-4      # the reference's own tolerance (tests/common/assert.rs:4)
    again.destroy(); buf.destroy()


def test_ply_file_round_trip_of_quaternions_normalised_once(gs, device, stream):
    """The general case next to the exact one above: quaternions as a loader leaves them, normalised once.  Reading them back
    divides by a computed length again.  Bound: a once-normalised q has |q|^2 = 1 + e with |e| <= 4 x 2^-24 (the roundings of
    the four products, three sums, the square root and the division of the first pass); the second pass computes its length
    with three more roundings of that size, so it divides by 1 + d with |d| < 2^-21 and rounds once: a component moves by
    less than 2^-21 of its value, and an ulp is at least 2^-24 of the value — 8 ulp.  Everything else as above."""
    n = 1500
    pod = gs.GaussianPod(0, 0)
    g = np.array(golden_export().scene(n + 2000)[1100:1100 + n])
    assert np.isfinite(g["rot"]).all()
    buf = gs.GaussiansBuffer.new(device, pod, g)
    before = buf.download(stream).view(np.uint32).reshape(n, 56)
    ply = gs.PlyGaussians.read_from(buf.write(stream, gs.GaussiansSource.Ply))
    again = gs.GaussiansBuffer.new_from_ply(device, pod, ply)
    after = again.download(stream).view(np.uint32).reshape(n, 56)
    assert np.array_equal(after[:, 0:3], before[:, 0:3]) and np.array_equal(after[:, 4:49], before[:, 4:49])

    def ordered(bits):
        b = bits.astype(np.int64)
        return np.where(b & 0x80000000, -(b & 0x7fffffff), b)
    d = np.abs(ordered(after[:, 49:53]) - ordered(before[:, 49:53]))
    print("rotation: %d of %d quaternions move, by at most %d ulp" % (int((d > 0).any(axis=1).sum()), n, int(d.max())))
    assert d.max() <= 8
    again.destroy(); buf.destroy()


# ---- errors ----------------------------------------------------------------------------------------------------------

def _status_and_message(gs, status):
    info = gs._capi.ErrorInfo()
    gs._capi.load().gs_last_error(C.byref(info))
    return status, info.message


@pytest.mark.parametrize("layout", REFUSED)
def test_refused_layouts_return_the_error_of_download_gaussians(gs, device, stream, layout):
    lib = gs._capi.load()
    n = 65
    pod = gs.GaussianPod(*layout)
    buf = gs.GaussiansBuffer.new(device, pod, export_scene(n))
    g_out = np.zeros(n, dtype=gs.GAUSSIAN_DTYPE)
    want = _status_and_message(gs, lib.gs_gaussians_buffer_download_gaussians(buf._h, stream._h, g_out.ctypes.data, n))
    assert want[0] == gs.LossyConfigError.code
    out = np.full(n * 248 + 4096, 0xAB, dtype=np.uint8)
    count, size = C.c_uint64(), C.c_size_t()
    opt = gs.spz_options()
    calls = [lambda: lib.gs_gaussians_buffer_export_ply(buf._h, stream._h, None, 0, out.ctypes.data, n, C.byref(count)),
             lambda: lib.gs_gaussians_buffer_export_spz_decompressed(buf._h, stream._h, None, 0, C.byref(opt), out.ctypes.data, out.size, C.byref(size)),
             lambda: lib.gs_gaussians_buffer_export_spz(buf._h, stream._h, None, 0, None, out.ctypes.data, out.size, C.byref(size)),
             lambda: lib.gs_gaussians_buffer_write(buf._h, stream._h, None, 0, 1, out.ctypes.data, out.size, C.byref(size)),
             lambda: lib.gs_gaussians_buffer_write(buf._h, stream._h, None, 0, 2, out.ctypes.data, out.size, C.byref(size))]
    for call in calls:
        assert _status_and_message(gs, call()) == want
        assert (out == 0xAB).all(), "out is untouched"
    with pytest.raises(gs.LossyConfigError):
        buf.export_ply(stream)
    buf.destroy()


def test_short_capacity_is_an_invalid_argument_and_writes_nothing(gs, device, stream):
    lib = gs._capi.load()
    n = 300
    buf = gs.GaussiansBuffer.new(device, gs.GaussianPod(0, 0), export_scene(n))
    mask = np.arange(n) % 2 == 0
    sel = selection_from_mask(gs, device, stream, mask)
    k = int(mask.sum())
    out = np.full(n * 248 + 4096, 0xAB, dtype=np.uint8)
    count, size = C.c_uint64(), C.c_size_t()
    assert lib.gs_gaussians_buffer_export_ply(buf._h, stream._h, sel._h, 0, None, 0, C.byref(count)) == 0 and count.value == k
    assert lib.gs_gaussians_buffer_export_ply(buf._h, stream._h, sel._h, 0, out.ctypes.data, k - 1, C.byref(count)) == INVALID_ARGUMENT
    assert count.value == k and (out == 0xAB).all()
    opt = gs.spz_options()
    for fn, head in ((lib.gs_gaussians_buffer_export_spz_decompressed, (C.byref(opt),)), (lib.gs_gaussians_buffer_export_spz, (None,)),
                     (lib.gs_gaussians_buffer_write, (1,)), (lib.gs_gaussians_buffer_write, (2,))):
        args = (buf._h, stream._h, sel._h, 0) + head
        assert fn(*args, None, 0, C.byref(size)) == 0 and size.value > 16
        need = size.value
        assert fn(*args, out.ctypes.data, need - 1, C.byref(size)) == INVALID_ARGUMENT
        assert size.value == need and (out == 0xAB).all()
        assert fn(*args, out.ctypes.data, need, C.byref(size)) == 0 and size.value == need
        assert (out[need:] == 0xAB).all(), "nothing behind the size is written"
        out[:] = 0xAB
    # a selection of another length
    other = gs.Selection(device, n + 1)
    assert lib.gs_gaussians_buffer_export_ply(buf._h, stream._h, other._h, 0, out.ctypes.data, n, C.byref(count)) == INVALID_ARGUMENT
    assert (out == 0xAB).all()
    other.destroy(); sel.destroy(); buf.destroy()


def test_empty_buffer_exports_empty_files(gs, device, stream):
    buf = gs.GaussiansBuffer.new_empty(device, gs.GaussianPod(0, 0), 0)
    none = np.zeros(0, dtype=gs.GAUSSIAN_DTYPE)
    assert len(buf.export_ply(stream)) == 0
    assert buf.write(stream, gs.GaussiansSource.Ply) == gs.PlyGaussians.from_gaussians(none).write_to()
    assert buf.export_spz(stream).payload == gs.SpzGaussians.write_gaussians_decompressed(none)
    buf.destroy()


# ---- ordering --------------------------------------------------------------------------------------------------------

def test_export_is_ordered_behind_an_edit_on_another_stream(gs, device, stream):
    n = 3000
    s1, s2 = stream, device.create_stream()
    buf = gs.GaussiansBuffer.new(device, gs.GaussianPod(0, 0), export_scene(n))
    before = buf.download_gaussians(s1)
    e = gs.edit(transform=gs.model_transform_pod(pos=(0.5, -0.25, 1.5), rot=(0, 0, 0, 1), scale=(1.25,) * 3), opacity=(0.5, 0.1))
    buf.edit(s1, None, e)
    got_ply = buf.export_ply(s2)              # no host synchronisation in between
    s1.synchronize()
    edited = buf.download_gaussians(s1)
    assert (edited["pos"].view(np.uint32) != before["pos"].view(np.uint32)).any(axis=1).mean() > 0.9
    assert got_ply.pods.tobytes() == gs.gaussian_to_ply(edited).tobytes()
    buf.edit(s1, None, e)
    got_spz = buf.export_spz(s2)
    s1.synchronize()
    assert got_spz.payload == gs.SpzGaussians.write_gaussians_decompressed(buf.download_gaussians(s1))
    s2.synchronize()
    buf.destroy()
    s2.close()
