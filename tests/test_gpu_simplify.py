"""Simplify a buffer on the device: gs_gaussians_buffer_create_simplified against the float64 witness of
tests/simplify_np.py.  The cells, K and the cell plane are exact; a merged cell is within the witness's bound for any
summation shape, colour and opacity bytes within 1; a cell with one member is the host's conversion bit for bit; every
destination layout is the host's conversion of the (SH f32, cov f32) result; then the edges, ordering, ownership and the
argument checks."""
import ctypes as C

import numpy as np
import pytest

import simplify_np as sn
from frames import render_image
from helpers import same_bits
from records import diff
from records import rows as _rows
from scenes import ALL_LAYOUTS

pytestmark = pytest.mark.gpu

f32 = np.float32
N = 5003
WIDE = sn.WIDE
THREE_SOURCES = [(0, 0), (1, 2), (2, 1)]
_CACHE = {}


def set_pods(gs, sh, cov, n=N):
    """the first n Gaussians of the set packed for one layout: once per key, read-only"""
    key = (sh, cov, n)
    if key not in _CACHE:
        if "g" not in _CACHE:
            _CACHE["g"] = sn.unit_cube_gaussians(N)
        p = gs.GaussianPod(sh, cov).from_gaussian(_CACHE["g"][:n])
        p.setflags(write=False)
        _CACHE[key] = p
    return _CACHE[key]


witness, simplify, check_against_witness = sn.witness, sn.simplify, sn.check_against_witness      # shared with test_gpu_simplify_runs.py


# ---- cells and counts ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell_size", [0.25, 0.05, 2.0])
def test_cells_and_counts_are_exact(gs, device, stream, cell_size):
    pods = set_pods(gs, 0, 0)
    c = sn.cells(sn.decode(0, 0, pods)["pos"], cell_size)
    got, cell_of, K = simplify(gs, device, stream, (0, 0), pods, cell_size)
    assert K == c["K"] and np.array_equal(cell_of, c["cell_of"])
    assert got.size == K * gs.GaussianPod(0, 0).size
    if cell_size == 0.25:
        assert K <= 125 and c["count"].max() > 64, "runs cross wave and block edges"
    if cell_size == 2.0:
        assert K == 1 and c["count"][0] == N, "one cell holds everything: the long-run path"
    if cell_size == 0.05:
        assert (c["count"] == 1).sum() > 1000 and (c["count"] >= 2).sum() > 500


# ---- merged values -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell_size", [0.25, 0.05, 2.0])
@pytest.mark.parametrize("src", THREE_SOURCES)
def test_merged_values_are_within_the_witness_bound(gs, device, stream, src, cell_size):
    c, w, _ = check_against_witness(gs, device, stream, src, set_pods(gs, *src), cell_size)
    assert (w["m"] >= 2).any()


# ---- singletons ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src,dst", [((0, 0), (1, 2)), ((2, 1), (2, 0)), ((1, 2), (1, 2)), ((0, 0), (0, 0))])
def test_singletons_are_the_conversion_bit_for_bit(gs, device, stream, src, dst):
    pods = set_pods(gs, *src)
    spod, dpod = gs.GaussianPod(*src), gs.GaussianPod(*dst)
    c = sn.cells(sn.decode(*src, pods)["pos"], 1e-4)
    assert c["K"] == N and (c["count"] == 1).all(), "every cell has one member"
    got, cell_of, K = simplify(gs, device, stream, src, pods, 1e-4, dst)
    assert K == N and np.array_equal(cell_of, c["cell_of"])
    one, want = sn.expected_singletons(gs, spod, dpod, pods, c)
    assert len(one) == N and np.array_equal(_rows(got, dpod.size), want), diff(got, want.reshape(-1), dpod.size)


# ---- destination layouts -------------------------------------------------------------------------------------------------

def test_every_destination_is_the_conversion_of_the_wide_result(gs, device, stream):
    n, cs = 1025, 0.25
    pods = set_pods(gs, 0, 0, n)
    wide = gs.GaussianPod(*WIDE)
    c, w, ref = check_against_witness(gs, device, stream, (0, 0), pods, cs)
    merged = c["count"] >= 2
    assert merged.sum() > 20
    for dst in ALL_LAYOUTS:
        dpod = gs.GaussianPod(*dst)
        got, cell_of, K = simplify(gs, device, stream, (0, 0), pods, cs, dst)
        assert K == c["K"] and np.array_equal(cell_of, c["cell_of"])
        want = ref if dst == WIDE else wide.decompose(ref, dst[0]) if dst[1] == 0 else wide.convert(ref, dpod)
        have, want = _rows(got, dpod.size), _rows(want, dpod.size)
        assert np.array_equal(have[merged], want[merged]), (dst, int((have[merged] != want[merged]).any(axis=1).sum()))
        one, single = sn.expected_singletons(gs, gs.GaussianPod(0, 0), dpod, pods, c)
        assert np.array_equal(have[one], single), dst


@pytest.mark.parametrize("src", ALL_LAYOUTS)
def test_every_source_layout_against_the_witness(gs, device, stream, src):
    check_against_witness(gs, device, stream, src, set_pods(gs, *src, 1025), 0.25)


# ---- reproducible --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell_size", [0.25, 2.0])
def test_two_calls_give_identical_bytes(gs, device, stream, cell_size):
    pods = set_pods(gs, 1, 2)
    a = simplify(gs, device, stream, (1, 2), pods, cell_size, (0, 0))
    b = simplify(gs, device, stream, (1, 2), pods, cell_size, (0, 0))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_small_buffers(gs, device, stream, n):
    pods = set_pods(gs, 0, 0, n) if n else np.zeros(0, np.uint8)
    for cs in (0.5, 2.0):
        if n:
            check_against_witness(gs, device, stream, (0, 0), pods, cs)
        else:
            got, cell_of, K = simplify(gs, device, stream, (0, 0), pods, cs, (1, 2))
            assert K == 0 and got.size == 0 and cell_of.size == 0


def test_among_masks(gs, device, stream):
    pods = set_pods(gs, 0, 0)
    among = np.random.default_rng(6).random(N) < 0.3
    c, _, _ = check_against_witness(gs, device, stream, (0, 0), pods, 0.25, among)
    assert (c["cell_of"][~among] == sn.NOT_A_POINT).all() and c["count"].sum() == among.sum()
    got, cell_of, K = simplify(gs, device, stream, (0, 0), pods, 0.25, (2, 2), np.zeros(N, bool))
    assert K == 0 and got.size == 0 and (cell_of == sn.NOT_A_POINT).all(), "an empty mask: the valid length-0 buffer"


def test_positions_that_are_not_finite_are_dropped(gs, device, stream):
    n, places = 2100, (0, 63, 64, 1023, 1024)
    rows = np.array(_rows(set_pods(gs, 0, 0, n), 224))
    for at, bad, axis in zip(places, (np.nan, np.inf, -np.inf, np.nan, np.inf), (0, 1, 2, 1, 0)):
        rows[at, 4 * axis:4 * axis + 4] = np.array([bad], f32).view(np.uint8)
    pods = rows.reshape(-1)
    for cs in (0.25, 2.0):
        c, _, _ = check_against_witness(gs, device, stream, (0, 0), pods, cs)
        assert (c["cell_of"][list(places)] == sn.NOT_A_POINT).all() and c["count"].sum() == n - len(places)


def test_duplicates_transparent_cells_and_a_far_outlier(gs, device, stream):
    n = 1300
    rows = np.array(_rows(set_pods(gs, 0, 0, n), 224))
    rows[100:170] = rows[100]                       # 70 exact duplicates: one run longer than a wave
    pos = np.ascontiguousarray(rows[:, :12]).view(f32)
    c0 = sn.cells(pos, 0.25)
    big = int(np.argmax(c0["count"]))
    members = c0["order"][c0["first"][big]:c0["first"][big] + c0["count"][big]]
    rows[members, 15] = 0                           # a whole cell with opacity 0: the unit-weight fallback
    pods = rows.reshape(-1)
    c, w, got = check_against_witness(gs, device, stream, (0, 0), pods, 0.25)
    k = int(c["cell_of"][members[0]])
    assert w["unit"][k] and w["m"][k] == len(members) >= 2 and _rows(got, 224)[k, 15] == 0
    dup = int(c["cell_of"][100])
    assert w["m"][dup] >= 70
    # identical members: the merged position is theirs up to the bound, whatever else shares the cell was checked above
    only = rows[100:170].reshape(-1)
    c1, w1, got1 = check_against_witness(gs, device, stream, (0, 0), only, 0.25)
    assert c1["K"] == 1 and np.allclose(np.ascontiguousarray(_rows(got1, 224)[0, :12]).view(f32), pos[100], rtol=0, atol=1e-6)
    # one far outlier at 1000 x the extent: the grid keeps its resolution, the outlier is a singleton
    far = rows.copy()
    far[7, :12] = np.array([1000.0, 1000.0, 1000.0], f32).view(np.uint8)
    c2, _, _ = check_against_witness(gs, device, stream, (0, 0), far.reshape(-1), 0.25)
    assert c2["count"][c2["cell_of"][7]] == 1 and c2["cell_of"][7] == c2["K"] - 1 and c2["K"] > 30


# ---- ordering and ownership ----------------------------------------------------------------------------------------------

def test_simplify_is_ordered_behind_an_edit_on_another_stream(gs, device, stream):
    spod = gs.GaussianPod(1, 1)
    pods = set_pods(gs, 1, 1)
    s1, s2 = stream, device.create_stream()
    buf = gs.GaussiansBuffer.new_with_pods(device, spod, pods)
    s1.synchronize()
    e = gs.edit(transform=gs.model_transform_pod(pos=(0.5, -0.25, 1.5), rot=(0, 0, 0, 1), scale=(1.25,) * 3), opacity=(0.5, 0.1))
    buf.edit(s1, None, e)
    out, plane = buf.simplify(s2, 0.3, gs.GaussianPod(*WIDE), cell_of_out=True)      # no host synchronisation in between
    s1.synchronize()
    edited = buf.download(s1)
    assert (_rows(edited, spod.size) != _rows(pods, spod.size)).any(axis=1).mean() > 0.9
    d, c, w = witness(1, 1, edited, 0.3)
    assert out.len() == c["K"] and np.array_equal(plane.download(s2, np.uint32)[:N], c["cell_of"])
    sn.check_merged(out.download(s2), w)
    s2.synchronize()
    out.destroy(); plane.release(); buf.destroy()
    s2.close()


def test_a_simplified_buffer_renders_like_a_direct_upload(gs, device, stream):
    import synth
    n, W, H = 3000, 128, 128
    g = synth.scene(n, first=31)
    pod = gs.GaussianPod(0, 0)
    cam = gs.camera_look_at((0, 0, 0), (0, 0, -1), (0, 1, 0), float(np.deg2rad(60.0)), W, H)
    gt, mt = gs.gaussian_transform_pod(sh_deg=3), gs.model_transform_pod()
    src = gs.GaussiansBuffer.new_with_pods(device, pod, pod.from_gaussian(g))
    for spatial in (True, False):
        src.set_spatial_order(spatial)
        simp = src.simplify(stream, 0.2)
        assert 0 < simp.len() < n and simp.spatial_order() == src.spatial_order() == spatial
        direct = gs.GaussiansBuffer.new_with_pods(device, pod, simp.download(stream))
        direct.set_spatial_order(spatial)
        r_a, r_b = gs.Renderer(device), gs.Renderer(device)
        got, fr_a = render_image(gs, device, stream, r_a, simp, gt, mt, cam, W, H)
        want, fr_b = render_image(gs, device, stream, r_b, direct, gt, mt, cam, W, H)
        assert fr_b.visible > 100 and (fr_a.visible, fr_a.pairs) == (fr_b.visible, fr_b.pairs)
        assert same_bits(got, want)
        for o in (r_a, r_b, simp, direct):
            o.destroy()
    src.destroy()


# ---- arguments -----------------------------------------------------------------------------------------------------------

def test_argument_errors_create_nothing(gs, device, stream):
    lib = gs._capi.load()
    call = lib.gs_gaussians_buffer_create_simplified
    bad = gs.InvalidArgumentError.code
    n = 65
    pods = set_pods(gs, 1, 2, n)
    buf = gs.GaussiansBuffer.new_with_pods(device, gs.GaussianPod(1, 2), pods)
    plane = gs.Buffer(device, size=4 * n)
    marks = np.arange(n, dtype=np.uint32) + 7
    plane.write(stream, 0, marks)
    stream.synchronize()
    short_plane, short_sel = gs.Buffer(device, size=4 * n - 4), gs.Selection(device, n - 1)
    other = gs.Device(0)          # a second device object: its objects belong to another device
    foreign_sel, foreign_plane = gs.Selection(other, n), gs.Buffer(other, size=4 * n)

    def refused(src=buf._h, among=None, cs=0.5, dsh=0, dcov=1, cell_of=plane._h, out=True):
        h, count = C.c_void_p(1), C.c_uint64(7)
        rc = call(src, stream._h, among, cs, dsh, dcov, cell_of, C.byref(h) if out else None, C.byref(count))
        assert rc == bad and count.value == 0 and (not out or h.value is None), (rc, count.value, h.value)

    refused(src=None)
    refused(out=False)
    for dsh, dcov in ((4, 0), (-1, 0), (0, 3), (0, -1)):
        refused(dsh=dsh, dcov=dcov)
    for cs in (-1.0, float("nan"), float("inf"), 1e20):
        refused(cs=cs)
    refused(among=short_sel._h)
    refused(among=foreign_sel._h)
    refused(cell_of=short_plane._h)
    refused(cell_of=foreign_plane._h)
    with pytest.raises(gs.InvalidArgumentError):
        buf.simplify(stream, 0.5, among=short_sel)
    with pytest.raises(gs.InvalidArgumentError):
        buf.simplify(stream, 0.5, cell_of_out=short_plane)
    assert np.array_equal(plane.download(stream, np.uint32)[:n], marks), "the plane is untouched"
    assert np.array_equal(buf.download(stream), pods)
    # ... and the same arguments, valid, go through
    out, got_plane = buf.simplify(stream, 0.5, gs.GaussianPod(0, 1), cell_of_out=plane)
    assert got_plane is plane and out.len() == sn.cells(sn.decode(1, 2, pods)["pos"], 0.5)["K"]
    out.destroy()
    for o in (short_sel, foreign_sel):
        o.destroy()
    for o in (plane, short_plane, foreign_plane):
        o.release()
    buf.destroy(); other.close()
