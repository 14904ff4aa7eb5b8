"""Simplify on the device, the control flow of gs_simplify_kernels.h by construction: the run shapes of
simplify_np.RUN_SHAPES put runs of equal cell keys at every alignment against the waves of 64 sorted slots, the blocks of
256 and the 64-partial chunks of the long-run walk (tests/test_simplify_api.py proves which wave states and partial counts
the table holds); every cell of every shape is marked in turn for the unit-weight pass; the two other triggers of that pass,
the 12 layouts under it, and the three regimes of the grid side.  Everything is compared as tests/test_gpu_simplify.py
compares (K and the cell plane exact, merged cells within the witness's bound, lone members bit for bit), and every value
of every merged cell is compared: the witness is finite throughout (require_finite)."""
import numpy as np
import pytest

import simplify_np as sn
from records import rows as _rows
from scenes import ALL_LAYOUTS

pytestmark = pytest.mark.gpu

f32 = np.float32
WIDE = sn.WIDE
POOL = 5003
_CACHE = {}


def pool():
    """the Gaussians every input here is cut from (the set of tests/test_gpu_simplify.py), every opacity byte >= 1: a cell
    takes the unit-weight pass only where a test marks it.  Once, read-only."""
    if "pool" not in _CACHE:
        g = sn.unit_cube_gaussians(POOL)
        g["color"][:, 3] = np.maximum(g["color"][:, 3], 1)
        g.setflags(write=False)
        _CACHE["pool"] = g
    return _CACHE["pool"]


def shape_pods(gs, name, layout=WIDE):
    """(records of a run shape packed for one layout, among, cells): once per key, read-only"""
    key = (name, layout)
    if key not in _CACHE:
        pos, among, counts = sn.run_shape(name)
        g = pool()[:len(pos)].copy()
        g["pos"] = pos
        p = gs.GaussianPod(*layout).from_gaussian(g)
        p.setflags(write=False)
        c = sn.cells(pos, sn.RUN_CELL, among)
        assert np.array_equal(c["count"], counts)
        _CACHE[key] = (p, among, c)
    return _CACHE[key]


def members(c, k):
    return c["order"][c["first"][k]:c["first"][k] + c["count"][k]]


def transparent(pods, size, c, marked):
    """a copy of the records with the opacity byte of every member of the marked cells 0: the weights of such a cell sum
    to 0, which is not > 0"""
    rows = np.array(_rows(pods, size))
    for k in marked:
        rows[members(c, k), 15] = 0
    return rows.reshape(-1)


def unit_is(w, marked):
    want = np.isin(np.arange(w["K"]), list(marked))
    assert np.array_equal(w["unit"], want), (np.flatnonzero(w["unit"]).tolist(), sorted(marked))


# ---- every shape -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sn.RUN_SHAPES))
def test_every_run_shape_against_the_witness(gs, device, stream, name):
    pods, among, c0 = shape_pods(gs, name)
    c, w, _ = sn.check_against_witness(gs, device, stream, WIDE, pods, sn.RUN_CELL, among, require_finite=True)
    assert np.array_equal(c["count"], c0["count"])
    unit_is(w, ())


@pytest.mark.parametrize("name", list(sn.RUN_SHAPES))
def test_every_cell_of_every_shape_through_the_unit_weight_pass(gs, device, stream, name):
    """no cell (above), each cell in turn, all cells: a marked run beside an unmarked one in every order, marked and
    unmarked partials in one wave (shape k), marked long runs of 64 / 65 / 66 partials, waves that return early"""
    pods, among, c0 = shape_pods(gs, name)
    K = c0["K"]
    for marked in [(k,) for k in range(K)] + [tuple(range(K))]:
        c, w, got = sn.check_against_witness(gs, device, stream, WIDE, transparent(pods, 224, c0, marked), sn.RUN_CELL, among,
                                             require_finite=True)
        unit_is(w, marked)
        merged = np.flatnonzero((c["count"] >= 2) & w["unit"])
        assert (_rows(got, 224)[merged, 15] == 0).all(), "the mean of opacities 0"


# ---- the other two triggers of the unit-weight pass ------------------------------------------------------------------

def with_covariances(gs, name, change):
    """the (SH f32, cov f32) records of a shape with change(cov float32[n, 6], cells) applied to the covariance words"""
    pods, among, c = shape_pods(gs, name)
    d = sn.decode(*WIDE, pods)
    d = dict(d, cov=d["cov"].copy())
    change(d["cov"], c)
    return sn.pack_wide(d), among


@pytest.mark.parametrize("name,k", [("g", 0), ("g", 1), ("h", 1), ("i", 1)])
def test_a_weight_that_is_not_finite_in_binary32_marks_its_cell(gs, device, stream, name, k):
    """one member with covariance diagonal 1.5e38 each: the trace overflows binary32, the weight is not finite; the unit
    sums (1.5e38 once, m >= 10 members) stay finite.  g 0: a run inside a wave; g 1: four partials; h 1, i 1: the long walk"""
    def change(cov, c):
        cov[members(c, k)[c["count"][k] // 2]] = (1.5e38, 0.0, 0.0, 1.5e38, 0.0, 1.5e38)
    pods, among = with_covariances(gs, name, change)
    c, w, got = sn.check_against_witness(gs, device, stream, WIDE, pods, sn.RUN_CELL, among, require_finite=True)
    unit_is(w, (k,))
    values = np.delete(_rows(got, 224)[:, :220], np.s_[12:16], axis=1)      # position, SH and covariance words
    assert np.isfinite(np.ascontiguousarray(values).view(f32)).all()


@pytest.mark.parametrize("name,marked", [("g", (0,)), ("g", (1,)), ("k", (1, 2)), ("j", (1,))])
def test_a_weight_sum_that_is_negative_marks_its_cell(gs, device, stream, name, marked):
    """every member of the marked cells has a negative covariance diagonal: W < 0 by far (no cancellation: every weight is
    negative)"""
    def change(cov, c):
        for k in marked:
            m = members(c, k)
            cov[m[:, None], [0, 3, 5]] = -np.maximum(np.abs(cov[m[:, None], [0, 3, 5]]), f32(1e-3))
    pods, among = with_covariances(gs, name, change)
    c, w, _ = sn.check_against_witness(gs, device, stream, WIDE, pods, sn.RUN_CELL, among, require_finite=True)
    unit_is(w, marked)


# ---- the 12 layouts under the unit-weight pass -----------------------------------------------------------------------

MARKED_G = (0, 1)      # shape g: a marked run inside a wave, a marked run of four partials, an unmarked run behind them


@pytest.mark.parametrize("src", ALL_LAYOUTS)
def test_every_source_layout_through_the_unit_weight_pass(gs, device, stream, src):
    pods, among, c0 = shape_pods(gs, "g", src)
    pods = transparent(pods, gs.GaussianPod(*src).size, c0, MARKED_G)
    c, w, _ = sn.check_against_witness(gs, device, stream, src, pods, sn.RUN_CELL, among, require_finite=True)
    unit_is(w, MARKED_G)


def test_every_destination_of_the_unit_weight_pass_is_the_conversion_of_the_wide_result(gs, device, stream):
    pods, among, c0 = shape_pods(gs, "g", (0, 0))
    pods = transparent(pods, gs.GaussianPod(0, 0).size, c0, MARKED_G)
    wide = gs.GaussianPod(*WIDE)
    c, w, ref = sn.check_against_witness(gs, device, stream, (0, 0), pods, sn.RUN_CELL, among, require_finite=True)
    unit_is(w, MARKED_G)
    assert (c["count"] >= 2).all()
    for dst in ALL_LAYOUTS:
        dpod = gs.GaussianPod(*dst)
        got, cell_of, K = sn.simplify(gs, device, stream, (0, 0), pods, sn.RUN_CELL, dst, among)
        assert K == c["K"] and np.array_equal(cell_of, c["cell_of"])
        want = ref if dst == WIDE else wide.decompose(ref, dst[0]) if dst[1] == 0 else wide.convert(ref, dpod)
        have, want = _rows(got, dpod.size), _rows(want, dpod.size)
        assert np.array_equal(have, want), (dst, np.flatnonzero((have != want).any(axis=1)).tolist())


# ---- reproducible ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["h", "i", "j"])
def test_two_calls_with_marked_long_cells_give_identical_bytes(gs, device, stream, name):
    pods, among, c0 = shape_pods(gs, name)
    pods = transparent(pods, 224, c0, range(c0["K"]))
    a = sn.simplify(gs, device, stream, WIDE, pods, sn.RUN_CELL, (0, 0), among)
    b = sn.simplify(gs, device, stream, WIDE, pods, sn.RUN_CELL, (0, 0), among)
    assert a[2] == b[2] == c0["K"] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the three regimes of the grid side ------------------------------------------------------------------------------
# h = max(cell_size (1 + 2^-10), extent 2^-21 (1 + 2^-10), 2^-62)

def cube_rows(gs, n):
    return np.array(_rows(gs.GaussianPod(0, 0).from_gaussian(pool()[:n]), 224))


@pytest.mark.parametrize("cell_size", [0.0, 1e-7])
def test_a_cell_size_below_the_resolution_of_the_extent(gs, device, stream, cell_size):
    """the second regime: the side is extent 2^-21; only identical positions share a cell"""
    rows = cube_rows(gs, 3000)
    rows[100:140, :12] = rows[100, :12]
    c, w, _ = sn.check_against_witness(gs, device, stream, (0, 0), rows.reshape(-1), cell_size, require_finite=True)
    assert c["h"] > 4 * max(cell_size, 2.0 ** -62) and c["K"] == 2961
    assert c["count"].max() == 40 and (c["count"] >= 2).sum() == 1 and c["count"][c["cell_of"][100]] == 40


def test_identical_positions_and_cell_size_zero(gs, device, stream):
    """the third regime: extent 0 and cell size 0, the side is 2^-62; one run over four waves"""
    rows = cube_rows(gs, 200)
    rows[:, :12] = rows[17, :12]
    c, w, got = sn.check_against_witness(gs, device, stream, (0, 0), rows.reshape(-1), 0.0, require_finite=True)
    assert c["h"] == 2.0 ** -62 and c["K"] == 1 and c["count"][0] == 200
    assert np.array_equal(_rows(got, 224)[0, :12], rows[17, :12]), "the mean of one position is that position"


def test_an_outlier_that_sets_the_cell_side(gs, device, stream):
    """the second regime above a cell size that is not 0: one Gaussian at 1e6 makes extent 2^-21 = 0.48 the side"""
    rows = cube_rows(gs, 3000)
    rows[7, :12] = np.array([1e6, 1e6, 1e6], f32).view(np.uint8)
    c, w, _ = sn.check_against_witness(gs, device, stream, (0, 0), rows.reshape(-1), 0.25, require_finite=True)
    assert 0.47 < c["h"] < 0.48 and c["h"] > 0.25 * (1.0 + 2.0 ** -10)
    assert c["K"] <= 28 and c["cell_of"][7] == c["K"] - 1 and c["count"][-1] == 1 and (c["count"] >= 2).sum() > 15
