"""The returns of the C ABI that happen while a call holds temporary device memory, events or a helper stream (DESIGN.md
§4.6, the scoped owners of csrc/gs_host.h): a refused call must leave the buffer, the stream and the device as they were.
Each refusal is followed by the same call with enough room, on the same buffer and stream, which must give the bytes the
existing tests define: tests/test_gpu_export.py for the exports (to_ply of the records, the host SPZ encoders),
tests/test_gpu_deflate.py for the gzip member (gs_gzip_fast of the same bytes), tests/test_gpu_history.py for a restore
(numpy indexing) and tests/test_gpu_convert.py for a conversion (the host conversion of the selected rows).

3 000 records of SH f32 / rot-scale: three 1024-blocks, the last one partial; every third record selected.  The sliced PLY
export (two staging buffers, events, a copy stream) is the GS3D_EXPORT_SLICE child of tests/test_gpu_export.py.

The handle objects hold their members in the same owners: the last tests destroy a renderer whose frame is only enqueued,
destroy a buffer, a selection, a snapshot and a renderer with every lazily created member alive (three cycles that must
agree byte for byte), and toggle the timing events."""
import ctypes as C

import numpy as np
import pytest

from frames import Scene
from helpers import same_bits
from records import selection_from_mask
from scenes import export_scene

pytestmark = pytest.mark.gpu

N = 3000
INVALID_ARGUMENT = -1
FILL = 0xAB


@pytest.fixture(scope="module")
def case(gs, device):
    """the buffer, its selection and what every export of the selected records must give: computed once, read-only"""
    st = device.create_stream()
    mask = np.arange(N) % 3 == 0
    buf = gs.GaussiansBuffer.new(device, gs.GaussianPod(0, 0), export_scene(N))
    sel = selection_from_mask(gs, device, st, mask)
    picked = buf.download_gaussians(st)[mask]
    ply = gs.gaussian_to_ply(picked)
    payload = gs.SpzGaussians.write_gaussians_decompressed(picked)
    want = {"ply": ply.tobytes(), "spz_decompressed": bytes(payload), "spz": bytes(gs.SpzGaussians.write_gaussians(picked)),
            "spz_fast": bytes(gs.gzip_fast(payload)), "ply_file": bytes(gs.PlyGaussians(ply).write_to())}
    yield buf, sel, mask, want
    st.synchronize()
    sel.destroy(); buf.destroy(); st.close()


def _refused_then_served(call, want, what):
    """call(out_pointer, capacity, size_ref) -> status: the size query, one byte short (refused, nothing written, the size
    still reported), then enough room: the bytes of `want` and nothing behind them"""
    out = np.full(len(want) + 4096, FILL, np.uint8)
    size = C.c_size_t()
    assert call(None, 0, C.byref(size)) == 0 and size.value == len(want), what
    assert call(out.ctypes.data, len(want) - 1, C.byref(size)) == INVALID_ARGUMENT, what
    assert size.value == len(want) and (out == FILL).all(), what
    assert call(out.ctypes.data, len(want), C.byref(size)) == 0 and size.value == len(want), what
    assert out[:len(want)].tobytes() == want, what
    assert (out[len(want):] == FILL).all(), what


def test_export_ply_short_capacity_then_enough(gs, stream, case):
    lib = gs._capi.load()
    buf, sel, mask, want = case
    k = int(mask.sum())
    out = np.full(k * 248 + 4096, FILL, np.uint8)
    count = C.c_uint64()
    assert lib.gs_gaussians_buffer_export_ply(buf._h, stream._h, sel._h, 0, out.ctypes.data, k - 1, C.byref(count)) == INVALID_ARGUMENT
    assert count.value == k and (out == FILL).all()
    assert lib.gs_gaussians_buffer_export_ply(buf._h, stream._h, sel._h, 0, out.ctypes.data, k, C.byref(count)) == 0 and count.value == k
    assert out[:k * 248].tobytes() == want["ply"] and (out[k * 248:] == FILL).all()


@pytest.mark.parametrize("entry,head,key", [("gs_gaussians_buffer_export_spz_decompressed", (None,), "spz_decompressed"),
                                            ("gs_gaussians_buffer_export_spz", (None,), "spz"),
                                            ("gs_gaussians_buffer_export_spz_fast", (None,), "spz_fast"),
                                            ("gs_gaussians_buffer_write", (1,), "ply_file"),
                                            ("gs_gaussians_buffer_write", (2,), "spz")])
def test_export_short_capacity_then_enough(gs, stream, case, entry, head, key):
    buf, sel, _, want = case
    fn = getattr(gs._capi.load(), entry)
    _refused_then_served(lambda out, cap, size: fn(buf._h, stream._h, sel._h, 0, *head, out, cap, size), want[key], (entry, head))


def test_gzip_fast_short_capacity_then_enough(gs, device, stream, case):
    """the member of the records themselves: 3 000 x 224 bytes, 21 chunks, the last one short"""
    lib = gs._capi.load()
    buf = case[0]
    data = buf.download(stream).tobytes()
    handle = lib.gs_gaussians_buffer_buffer(buf._h)      # (borrowed: the Gaussian buffer keeps it)
    _refused_then_served(lambda out, cap, size: lib.gs_buffer_gzip_fast(handle, stream._h, 0, len(data), out, cap, size),
                         bytes(gs.gzip_fast(data)), "gs_buffer_gzip_fast")


def test_restore_of_another_layout_then_one_that_fits(gs, device, stream, case):
    lib = gs._capi.load()
    _, sel, mask, _ = case
    pod, other_pod = gs.GaussianPod(0, 0), gs.GaussianPod(0, 2)
    A = np.asarray(pod.from_gaussian(export_scene(N))).reshape(N, pod.size)
    B = A[::-1].copy()
    a = gs.GaussiansBuffer.new_with_pods(device, pod, A)
    b = gs.GaussiansBuffer.new_with_pods(device, pod, B)
    other = gs.GaussiansBuffer.new(device, other_pod, export_scene(N))
    before = other.download(stream).copy()
    snap = C.c_void_p()
    assert lib.gs_gaussians_buffer_snapshot(a._h, stream._h, sel._h, C.byref(snap)) == 0 and lib.gs_snapshot_count(snap) == int(mask.sum())
    for exchange in (0, 1):
        assert lib.gs_gaussians_buffer_restore(other._h, stream._h, snap, exchange) == INVALID_ARGUMENT
    assert np.array_equal(other.download(stream), before)
    assert lib.gs_gaussians_buffer_restore(b._h, stream._h, snap, 0) == 0
    got = np.asarray(b.download(stream)).reshape(N, pod.size)
    assert np.array_equal(got, np.where(mask[:, None], A, B))
    stream.synchronize()
    lib.gs_snapshot_destroy(snap)
    for o in (other, b, a):
        o.destroy()


@pytest.mark.parametrize("dst", [(0, 0), (1, 2)])
def test_empty_selection_then_a_selection(gs, device, stream, case, dst):
    """extraction (the layouts agree) and conversion: a total of 0 creates the valid empty buffer, the next call the records"""
    lib = gs._capi.load()
    buf, sel, mask, _ = case
    spod, dpod = gs.GaussianPod(0, 0), gs.GaussianPod(*dst)
    rows = np.asarray(buf.download(stream)).reshape(N, spod.size)
    empty = selection_from_mask(gs, device, stream, np.zeros(N, bool))

    def create(selection):
        h, count = C.c_void_p(), C.c_uint64(77)
        if dst == (0, 0):
            rc = lib.gs_gaussians_buffer_create_from_selection(buf._h, stream._h, selection._h, 0, C.byref(h), C.byref(count))
        else:
            rc = lib.gs_gaussians_buffer_create_converted(buf._h, stream._h, selection._h, 0, dst[0], dst[1], C.byref(h), C.byref(count))
        assert rc == 0 and h.value is not None
        assert (lib.gs_gaussians_buffer_sh(h), lib.gs_gaussians_buffer_cov3d(h)) == dst
        return h, count.value

    h, count = create(empty)
    assert count == 0 and lib.gs_gaussians_buffer_len(h) == 0
    lib.gs_gaussians_buffer_destroy(h)
    h, count = create(sel)
    k = int(mask.sum())
    assert count == k and lib.gs_gaussians_buffer_len(h) == k
    got = np.zeros(k * dpod.size, np.uint8)
    assert lib.gs_gaussians_buffer_download(h, stream._h, got.ctypes.data, k) == 0
    want = spod.convert(np.ascontiguousarray(rows[mask]).reshape(-1), dpod)
    assert np.array_equal(got, np.asarray(want).reshape(-1))
    lib.gs_gaussians_buffer_destroy(h)
    empty.destroy()


# ---- the handle objects: their members are owners too, and gs_*_destroy is a wait and a delete ----

ENQ_N, ENQ_W, ENQ_H = 2000, 64, 48
NB_RADIUS = 0.25      # of the neighbour counts: asserted to find neighbours in the 3 000 Gaussians of synth.scene


@pytest.fixture(scope="module")
def enqueued_frame_oracle(gs, ob, device):
    """the oracle's image of the scene the two destroy-while-enqueued cases render: computed once, read-only"""
    st = device.create_stream()
    sc = Scene(gs, ob, device, st, gs.SH_NONE, gs.COV3D_ROT_SCALE, ENQ_N, ENQ_W, ENQ_H)
    rgba = np.ascontiguousarray(sc.oracle(sc.pods)["rgba"], np.float32).reshape(ENQ_H, ENQ_W, 4)
    rgba.setflags(write=False)
    sc.release()
    st.close()
    return rgba


@pytest.mark.parametrize("close_stream_first", [False, True])
def test_renderer_destroyed_with_its_frame_only_enqueued(gs, ob, device, stream, enqueued_frame_oracle, close_stream_first):
    """gs_renderer_destroy waits for the frame before the pinned results, the scratch and the events (timing events
    included) go: through the stream, or — the stream was closed first — through the end-of-frame event"""
    st = device.create_stream()
    sc = Scene(gs, ob, device, st, gs.SH_NONE, gs.COV3D_ROT_SCALE, ENQ_N, ENQ_W, ENQ_H)
    r = gs.Renderer(device)
    r.set_timing(True)
    r.render(st, sc.buf, sc.gt, sc.mt, sc.cam, sc.img.device_ptr(), check=False)
    if close_stream_first:
        st.close()
    r.destroy()
    got = sc.img.download(stream, np.float32).reshape(ENQ_H, ENQ_W, 4)
    assert same_bits(got, enqueued_frame_oracle)
    sc.release()
    if not close_stream_first:
        st.close()


def _handle_cycle(gs, ob, device, stream):
    """every lazily created member of a buffer, a selection and a renderer alive, then all of them destroyed"""
    sc = Scene(gs, ob, device, stream, gs.SH_NONE, gs.COV3D_ROT_SCALE, N, ENQ_W, ENQ_H)
    assert sc.buf.spatial_order()
    r = gs.Renderer(device)
    sc.render(r)                                                  # mirror, order, inverse, block bounds, mirror_ready
    out = {"image": sc.image().tobytes(), "order": sc.order().tobytes()}
    sel = gs.Selection(device, N)
    r.select_visible(stream, sel, 0, 0, ENQ_W, ENQ_H)             # the selection's scratch plane
    out["count"] = sel.count(stream)                              # ... and its counter
    out["selection"] = np.asarray(sel.download(stream)).tobytes()
    assert 0 < out["count"] < N
    sc.buf.edit(stream, sel, gs.edit(color=gs.color_override((1, 0.5, 0))))      # edit_done
    s = sc.buf.stats(stream)                                      # stats_scratch
    out["stats"] = (s.count, s.finite.tobytes(), s.min.tobytes(), s.max.tobytes(), s.sum.tobytes())
    plane = sc.buf.neighbor_counts(stream, NB_RADIUS)             # nb_scratch, nb_done
    counts = plane.download(stream, np.uint32)[:N].copy()
    plane.release()
    assert counts.max() > 0, "the radius finds no neighbours"
    out["neighbours"] = counts.tobytes()
    snap = sc.buf.snapshot(stream, sel)
    out["snapshot"] = (snap.count, snap.nbytes)
    assert snap.count == out["count"]
    out["records"] = np.asarray(sc.buf.download(stream)).tobytes()
    assert out["records"] != np.asarray(sc.pods).tobytes(), "the colour edit changed nothing"
    stream.synchronize()
    snap.destroy()
    sel.destroy()
    r.destroy()
    sc.release()
    return out


def test_handles_destroyed_with_every_lazy_member_alive_three_cycles(gs, ob, device, stream):
    first = _handle_cycle(gs, ob, device, stream)
    for cycle in (2, 3):
        again = _handle_cycle(gs, ob, device, stream)
        for key, want in first.items():
            assert again[key] == want, "cycle %d: %s differs from cycle 1" % (cycle, key)


def test_timing_toggled_around_two_frames(gs, ob, device, stream):
    """the timing events are made once, by the first set_timing(True); only frames rendered while it is on are counted"""
    sc = Scene(gs, ob, device, stream, gs.SH_NONE, gs.COV3D_ROT_SCALE, ENQ_N, ENQ_W, ENQ_H)
    r = gs.Renderer(device)
    r.set_timing(True)
    sc.render(r)
    r.set_timing(False)
    sc.render(r)
    r.set_timing(True)
    st = r.stats()
    assert st.timed_frames == 1
    assert st.stage_ms[8] > 0.0      # ST_FRAME: the whole timed frame
    r.destroy()
    sc.release()
