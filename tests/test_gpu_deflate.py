"""The Huffman-only gzip member deflated on the device: Buffer.gzip_fast against the host encoder gs_gzip_fast,
byte for byte, over the inputs of tests/test_deflate_api.py (the smallest shapes at which a piece, a chunk or a gather boundary
can go wrong), at unaligned offsets and over 41 chunks; export_spz_fast against the payload of export_spz_decompressed for
every selection shape, the three layouts that can be exported and two option sets; the refused layouts, a short capacity and
a range past the buffer."""
import ctypes as C
import gzip

import numpy as np
import pytest

import deflate_np
from records import first_difference, selection_from_mask
from scenes import deflate_selections, export_scene

pytestmark = pytest.mark.gpu

EXPORTABLE = [(0, 0), (1, 0), (2, 0)]
REFUSED = [(s, c) for s in range(4) for c in range(3) if (s, c) not in EXPORTABLE]
SIZES = [1, 64, 1025, 3000]
NAMES = [name for name, _ in deflate_np.inputs()]


@pytest.fixture(scope="module")
def host_members(gs):
    """{name: (input, gs_gzip_fast of it)}: the reference, computed once"""
    return {name: (data, gs.gzip_fast(data)) for name, data in deflate_np.inputs()}


@pytest.mark.parametrize("name", NAMES)
def test_device_member_equals_the_host_member(gs, device, stream, host_members, name):
    data, want = host_members[name]
    buf = gs.Buffer(device, data=np.frombuffer(data + b"\xa5", np.uint8))      # one byte behind the range: never read into the member
    got = buf.gzip_fast(stream, 0, len(data))
    assert got == want, (name, first_difference(got, want))
    # the size query runs the same kernels without the gather
    n = C.c_size_t()
    assert gs._capi.load().gs_buffer_gzip_fast(buf._h, stream._h, 0, len(data), None, 0, C.byref(n)) == 0
    assert n.value == len(want)
    buf.release()


@pytest.mark.parametrize("offset", [1, 2, 3, 13])
def test_unaligned_offsets(gs, device, stream, host_members, offset):
    for name in ("skewed_98309", "three_forms", "skewed_129"):
        data, want = host_members[name]
        buf = gs.Buffer(device, data=np.frombuffer(bytes(range(1, offset + 1)) + data + b"\x77\x77", np.uint8))
        got = buf.gzip_fast(stream, offset, len(data))
        assert got == want, (name, offset, first_difference(got, want))
        buf.release()


def test_forty_one_chunks(gs, device, stream):
    """every form several times over, the last chunk short: the offsets of the size scan are carried from thread to thread, and
    the gather places 41 images of very different sizes at every byte alignment"""
    rng = np.random.default_rng(41)
    parts = []
    for k in range(41):
        kind = k % 4
        n = 32768 if k < 40 else 32768 - 1234
        if kind == 0:
            parts.append(deflate_np.skewed(n, 400 + k))
        elif kind == 1:
            parts.append(bytes([k]) * n)
        elif kind == 2:
            parts.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        else:
            parts.append(np.where(rng.random(n) < 0.2, 3, 0).astype(np.uint8).tobytes())
    data = b"".join(parts)
    want = gs.gzip_fast(data)
    assert gzip.decompress(want) == data
    buf = gs.Buffer(device, data=np.frombuffer(data, np.uint8))
    got = buf.gzip_fast(stream)
    assert got == want, first_difference(got, want)
    buf.release()


def test_range_and_capacity_errors(gs, device, stream, host_members):
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    data, want = host_members["skewed_32769"]
    buf = gs.Buffer(device, data=np.frombuffer(data, np.uint8))
    out = np.full(len(want), 0xee, np.uint8)
    n = C.c_size_t()
    assert lib.gs_buffer_gzip_fast(buf._h, stream._h, 0, len(data) + 1, out.ctypes.data, out.size, C.byref(n)) == bad
    assert lib.gs_buffer_gzip_fast(buf._h, stream._h, len(data) + 1, 0, out.ctypes.data, out.size, C.byref(n)) == bad
    assert lib.gs_buffer_gzip_fast(buf._h, stream._h, 2, len(data) - 1, out.ctypes.data, out.size, C.byref(n)) == bad
    assert lib.gs_buffer_gzip_fast(buf._h, stream._h, 0, len(data), out.ctypes.data, len(want) - 1, C.byref(n)) == bad
    assert n.value == len(want) and (out == 0xee).all()
    assert lib.gs_buffer_gzip_fast(buf._h, stream._h, 0, len(data), out.ctypes.data, out.size, None) == bad and (out == 0xee).all()
    assert lib.gs_buffer_gzip_fast(buf._h, stream._h, 0, len(data), out.ctypes.data, out.size, C.byref(n)) == 0 and out.tobytes() == want
    assert buf.gzip_fast(stream, len(data), 0) == gs.gzip_fast(b"")      # an empty range at the very end
    buf.release()


@pytest.mark.parametrize("layout", EXPORTABLE)
def test_export_round_trip(gs, device, stream, layout):
    pod = gs.GaussianPod(*layout)
    done = 0
    for n in SIZES:
        buf = gs.GaussiansBuffer.new(device, pod, export_scene(n))
        for name, mask, invert in deflate_selections(n):
            sel = selection_from_mask(gs, device, stream, mask)
            keep = n if mask is None else int((~mask if invert else mask).sum())
            for version, degree in ((3, 3), (1, 0)):
                opt = gs.spz_options(version=version, sh_degree=degree)
                what = (layout, n, name, version, degree)
                payload = buf.export_spz(stream, sel, invert, opt).payload
                got = buf.export_spz_file(stream, sel, invert, opt, fast=True)
                assert gzip.decompress(got) == payload, what
                assert got == gs.gzip_fast(payload), (what, first_difference(got, gs.gzip_fast(payload)))
                hdr, back = gs.SpzGaussians.decode(got)
                assert len(back) == keep == hdr.num_points and hdr.version == version and hdr.sh_degree == degree, what
                assert back.tobytes() == gs.SpzGaussians(payload).gaussians.tobytes(), what
                done += 1
            if sel is not None:
                sel.destroy()
        # write(fast=True) is the fast export with the default options; the zlib path keeps its bytes
        fast = buf.write(stream, gs.GaussiansSource.Spz, fast=True)
        slow = buf.write(stream, gs.GaussiansSource.Spz)
        assert fast == buf.export_spz_file(stream) and gzip.decompress(fast) == gzip.decompress(slow) == buf.export_spz(stream).payload
        assert slow == buf.export_spz_file(stream, fast=False) == gs.SpzGaussians.write_gaussians(buf.download_gaussians(stream))
        buf.destroy()
    assert done == len(SIZES) * 4 * 2


def test_export_errors_are_those_of_the_zlib_export(gs, device, stream):
    lib = gs._capi.load()
    g = export_scene(64)
    out = np.full(1 << 16, 0xee, np.uint8)
    n = C.c_size_t()
    info = gs._capi.ErrorInfo()
    for layout in REFUSED:
        buf = gs.GaussiansBuffer.new(device, gs.GaussianPod(*layout), g)
        want = lib.gs_gaussians_buffer_export_spz(buf._h, stream._h, None, 0, None, out.ctypes.data, out.size, C.byref(n))
        lib.gs_last_error(C.byref(info))
        message = info.message
        got = lib.gs_gaussians_buffer_export_spz_fast(buf._h, stream._h, None, 0, None, out.ctypes.data, out.size, C.byref(n))
        lib.gs_last_error(C.byref(info))
        assert got == want != 0 and info.message == message and (out == 0xee).all(), layout
        buf.destroy()
    buf = gs.GaussiansBuffer.new(device, gs.GaussianPod(0, 0), g)
    bad = gs.InvalidArgumentError.code
    assert lib.gs_gaussians_buffer_export_spz_fast(buf._h, stream._h, None, 0, None, None, 0, C.byref(n)) == 0
    size = n.value
    assert size == len(buf.export_spz_file(stream))
    assert lib.gs_gaussians_buffer_export_spz_fast(buf._h, stream._h, None, 0, None, out.ctypes.data, size - 1, C.byref(n)) == bad
    assert lib.gs_gaussians_buffer_export_spz_fast(buf._h, stream._h, None, 0, None, out.ctypes.data, out.size, None) == bad
    other = gs.Selection(device, 63)      # a selection of another length
    assert lib.gs_gaussians_buffer_export_spz_fast(buf._h, stream._h, other._h, 0, None, out.ctypes.data, out.size, C.byref(n)) == bad
    badopt = gs.spz_options(version=4)
    assert lib.gs_gaussians_buffer_export_spz_fast(buf._h, stream._h, None, 0, C.byref(badopt), out.ctypes.data, out.size, C.byref(n)) \
        == lib.gs_gaussians_buffer_export_spz(buf._h, stream._h, None, 0, C.byref(badopt), out.ctypes.data, out.size, C.byref(n)) != 0
    assert (out == 0xee).all()
    other.destroy(); buf.destroy()
