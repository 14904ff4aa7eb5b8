"""Simplify a buffer, the parts that need no device: the header declares the entry point with its note and
in its place, the ctypes layer binds it, the Rust file and the C++ mirror name it, the Python layer refuses wrong arguments
before any library call, and the float64 witness of tests/simplify_np.py satisfies the identities of its own definition."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import simplify_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY = "gs_gaussians_buffer_create_simplified"
TITLE = "Simplify: merge the Gaussians of each grid cell into one"
f32, f64 = np.float32, np.float64


def test_header_declares_the_simplify_api(gs):
    text = open(os.path.join(ROOT, "include", "gs3d.h")).read()
    lib = gs._capi.load()
    assert lib.gs_abi_version() == 1
    assert re.search(r"\b%s\s*\(" % ENTRY, text)
    assert hasattr(lib, ENTRY), "the symbol is exported"
    vp = C.c_void_p
    assert gs._capi.SIGNATURES[ENTRY] == (C.c_int32, [vp, vp, vp, C.c_float, C.c_int32, C.c_int32, vp, vp, vp])
    assert getattr(lib, ENTRY).argtypes == gs._capi.SIGNATURES[ENTRY][1] and getattr(lib, ENTRY).restype == C.c_int32
    assert text.count(TITLE) == 1
    clusters = "Clusters: connected components within a radius, select by cluster size"
    assert text.index(clusters) < text.index("gs_select_connected(") < text.index(TITLE) < text.index("Stand-alone device primitives")
    section = text[text.index(TITLE):text.index("Stand-alone device primitives")]
    comment = section[:section.index(ENTRY + "(")]
    assert "no reference item" in comment and "DESIGN.md 3.17" in comment
    # the header states that the summation shape is not part of the definition, and the blocking round trip
    assert "THE SHAPE ITSELF IS NOT PART OF THE DEFINITION" in comment and "BLOCKING" in comment
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**3.17 " in design and ENTRY in design
    assert "gs_simplify.hip" in design and "gs_simplify.hip" in open(os.path.join(ROOT, "README.md")).read()
    build = open(os.path.join(ROOT, "wgpu-3dgs-core_amd", "build.py")).read()
    assert '"gs_simplify.hip"' in build


def test_rust_and_cpp_name_the_simplify_api():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    assert "pub fn %s(" % ENTRY in rs
    decl = rs[rs.index("pub fn %s(" % ENTRY):].split(";", 1)[0]
    assert "cell_size: f32" in decl and "cell_of_out: *mut gs_buffer" in decl and "count_out: *mut u64" in decl
    assert ENTRY in hpp and "simplify(Stream &s, float cell_size" in hpp


def _stand_in(cls, **attrs):
    """a handle-less object: nothing it is given to may reach the library"""
    o = object.__new__(cls)
    o._h = None
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_simplify_arguments_are_checked_without_a_device(gs):
    buf = _stand_in(gs.GaussiansBuffer, pod=gs.GaussianPod(0, 0), device=None)
    for bad in (-1.0, float("nan"), float("inf"), 1e20):          # 1e20 squared is not finite in binary32
        with pytest.raises(ValueError):
            buf.simplify(None, bad)
    for bad in ("1", None, True, (1.0,)):
        with pytest.raises(TypeError):
            buf.simplify(None, bad)
    with pytest.raises(TypeError):
        buf.simplify(None, 1.0, pod=(0, 1))
    with pytest.raises(TypeError):
        buf.simplify(None, 1.0, among=np.zeros(4, bool))
    with pytest.raises(TypeError):
        buf.simplify(None, 1.0, cell_of_out=np.zeros(4, np.uint32))
    p = inspect.signature(gs.GaussiansBuffer.simplify).parameters
    assert list(p)[1:] == ["stream", "cell_size", "pod", "among", "cell_of_out"]
    assert all(p[k].default is None for k in list(p)[3:])
    assert ENTRY in gs.GaussiansBuffer.simplify.__doc__


def test_null_arguments_are_errors_of_the_c_abi(gs):
    """no device is touched"""
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    h, count = C.c_void_p(1), C.c_uint64(7)
    assert lib.gs_gaussians_buffer_create_simplified(None, None, None, 1.0, 0, 0, None, C.byref(h), C.byref(count)) == bad
    assert h.value is None and count.value == 0
    assert lib.gs_gaussians_buffer_create_simplified(None, None, None, 1.0, 0, 0, None, None, None) == bad


# ---- the witness against its own definition ------------------------------------------------------------------------------

def _decoded(n, seed, size=1e-3):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, 3, 3))
    S = A @ A.transpose(0, 2, 1) * size
    cov = np.stack([S[:, a, b] for a, b in sn.COV_PAIRS], axis=1).astype(f32)
    rgba = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    return dict(pos=rng.random((n, 3)).astype(f32), rgba=rgba, sh=rng.uniform(-1, 1, (n, 45)).astype(f32), cov=cov)


def test_witness_cells_are_the_grid_of_the_definition():
    d = _decoded(400, 1)
    d["pos"][7, 1] = np.nan
    d["pos"][8, 0] = np.inf
    among = np.random.default_rng(2).random(400) < 0.7
    among[[7, 8]] = True
    for cs in (0.25, 0.05, 2.0, 0.0):
        c = sn.cells(d["pos"], cs, among)
        pt = c["pt"]
        assert not pt[7] and not pt[8] and (pt == (among & np.isfinite(d["pos"]).all(axis=1))).all()
        assert (c["cell_of"][~pt] == sn.NOT_A_POINT).all() and c["cell_of"][pt].max() == c["K"] - 1
        assert (np.diff(c["keys"].astype(np.uint64)) > 0).all(), "ascending keys, each once"
        assert c["count"].sum() == pt.sum() and (c["count"] > 0).all()
        # a point lies inside its cell up to the rounding of the quotient; the cell side is at least the cell size
        assert c["h"] >= cs
        lo_edge = c["lo"] + c["q"][pt] * c["h"]
        assert (d["pos"][pt] >= lo_edge - 1e-9).all() and (d["pos"][pt] <= lo_edge + c["h"] + 1e-9).all()
        # stable: inside a cell the members keep their caller order
        for k in range(c["K"]):
            run = c["order"][c["first"][k]:c["first"][k] + c["count"][k]]
            assert (np.diff(run) > 0).all() and (c["cell_of"][run] == k).all()
    assert sn.cells(d["pos"], 2.0)["K"] == 1
    none = sn.cells(d["pos"], 0.25, np.zeros(400, bool))
    assert none["K"] == 0 and (none["cell_of"] == sn.NOT_A_POINT).all()


def test_a_cell_of_identical_gaussians_returns_that_gaussian():
    d = _decoded(5, 3)
    for k in ("pos", "rgba", "sh", "cov"):
        d[k][:] = d[k][0]
    d["rgba"][:, 3] = 40      # opacity x size mass is kept: five copies of opacity 40 / 255 are one of 200 / 255
    c = sn.cells(d["pos"], 0.5)
    w = sn.merge(d, c)
    assert c["K"] == 1 and w["m"][0] == 5 and not w["unit"][0]
    assert np.allclose(w["pos"][0], d["pos"][0].astype(f64), rtol=0, atol=1e-12)
    assert np.allclose(w["cov"][0], d["cov"][0].astype(f64), rtol=1e-9, atol=1e-15)
    assert np.allclose(w["sh"][0], d["sh"][0].astype(f64), rtol=1e-12)
    assert (sn.color_bytes(w["rgb"][0]) == d["rgba"][0, :3]).all() and sn.color_bytes(w["alpha"][0]) == 200
    d["rgba"][:, 3] = 200      # ... saturating at 1
    assert sn.color_bytes(sn.merge(d, c)["alpha"][0]) == 255
    # ... and with opacity 0 everywhere the unit-weight fallback does the same, with the mean opacity
    d["rgba"][:, 3] = 0
    w = sn.merge(d, c)
    assert w["unit"][0] and sn.color_bytes(w["alpha"][0]) == 0
    assert np.allclose(w["cov"][0], d["cov"][0].astype(f64), rtol=1e-9, atol=1e-15) and np.allclose(w["pos"][0], d["pos"][0].astype(f64), atol=1e-12)


def test_merged_covariances_are_symmetric_positive_semidefinite_and_keep_the_mass():
    d = _decoded(3000, 4, size=1e-5)      # small against the cells: the merged opacity stays below 1
    d["rgba"][::7, 3] = 0
    c = sn.cells(d["pos"], 0.2)
    w = sn.merge(d, c)
    assert (w["m"] >= 2).sum() > 50
    M = np.zeros((c["K"], 3, 3))
    for k, (a, b) in enumerate(sn.COV_PAIRS):
        M[:, a, b] = M[:, b, a] = w["cov"][:, k]
    lam = np.linalg.eigvalsh(M)
    assert (lam[:, 0] >= -1e-12 * np.abs(lam[:, 2])).all()
    # opacity x size mass: alpha trace = W where nothing was clamped
    o = c["order"]
    alpha, size = d["rgba"][o, 3].astype(f64) / 255.0, d["cov"][o].astype(f64)[:, [0, 3, 5]].sum(axis=1)
    W = np.add.reduceat(alpha * size, c["first"])
    free = ~w["unit"] & (w["alpha"] < 1.0)
    assert free.sum() > 50 and np.allclose((w["alpha"] * w["cov"][:, [0, 3, 5]].sum(axis=1))[free], W[free], rtol=1e-9)
    # the position lies in the convex hull of its members, the bounds are positive and small
    for k in np.flatnonzero(w["m"] >= 2)[:40]:
        run = o[c["first"][k]:c["first"][k] + c["count"][k]]
        assert (w["pos"][k] >= d["pos"][run].min(axis=0) - 1e-12).all() and (w["pos"][k] <= d["pos"][run].max(axis=0) + 1e-12).all()
    assert (w["pos_tol"] > 0).all() and (w["pos_tol"] < 1e-4).all() and (w["cov_tol"] >= 0).all()


# ---- the constructed run shapes: what the table of simplify_np.RUN_SHAPES covers ------------------------------------------

def test_pack_wide_is_the_inverse_of_decode():
    d = _decoded(37, 5)
    back = sn.decode(0, 1, sn.pack_wide(d))
    assert all(np.array_equal(np.asarray(back[k]).view(np.uint8), np.asarray(d[k]).view(np.uint8)) for k in ("pos", "rgba", "sh", "cov"))
    assert sn.pack_wide(d).size == 37 * 224 and not sn.pack_wide(d).reshape(37, 224)[:, 220:].any()


def test_run_shapes_have_the_designed_counts_and_cover_every_wave_state():
    """The proof that tests/test_gpu_simplify_runs.py reaches what it claims: every shape has exactly the designed members
    per cell in sorted order, and over the whole table every pair (what came into a wave, what goes on from it) that can
    occur does occur, as do crossing runs of exactly 2, 64, 65 and 66 partials."""
    pairs, partials, per = set(), set(), {}
    for name, (counts, tail, _) in sn.RUN_SHAPES.items():
        pos, among, want = sn.run_shape(name)
        assert len(pos) == sum(counts) + tail and (among is None) == (tail == 0)
        c = sn.cells(pos, sn.RUN_CELL, among)
        assert c["K"] == len(counts) and np.array_equal(c["count"], want), (name, c["count"].tolist())
        assert c["h"] == float(f32(sn.RUN_CELL)) * (1.0 + 2.0 ** -10), "the first grid regime"
        assert not np.array_equal(c["order"], np.arange(len(c["order"]))), "the caller order is permuted"
        if tail:
            assert (~c["pt"]).sum() == tail and (c["cell_of"][~among] == sn.NOT_A_POINT).all()
        wp = sn.wave_partials(c)
        assert len(wp["incoming"]) == len(wp["outgoing"]) == (len(pos) + 63) // 64
        per[name] = list(zip(wp["incoming"], wp["outgoing"]))
        pairs |= set(per[name])
        partials |= set(int(x) for x in wp["partials"] if x >= 2)
    N_, O_, M_, L_ = sn.W_NONE, sn.W_OPEN, sn.W_MIDDLE, sn.W_LAST
    # (middle, open) cannot occur: a run that came in and goes on fills the wave, so no run starts in it
    assert pairs == {(N_, N_), (N_, O_), (L_, N_), (L_, O_), (M_, N_)}, pairs
    assert {2, 64, 65, 66} <= partials, sorted(partials)
    # ... and shape by shape what the table says of it
    assert per["a"] == [(N_, N_), (N_, N_)] and per["b"] == [(N_, N_)] * 3
    assert per["c"] == [(N_, O_), (L_, N_)] and per["d"][3:] == [(L_, O_), (L_, N_)]
    assert per["e"] == [(N_, N_), (N_, N_)]
    assert per["f"] == [(N_, N_), (N_, O_), (M_, N_), (L_, N_), (N_, N_)]
    assert per["g"] == [(N_, O_), (M_, N_), (M_, N_), (L_, N_)]
    for name, waves in (("h", 64), ("i", 65), ("j", 66)):
        assert per[name][0] == (N_, O_) and per[name][1:waves - 1] == [(M_, N_)] * (waves - 2) and per[name][waves - 1] == (L_, N_)
        assert len(per[name]) == waves
    assert per["k"] == [(N_, O_), (M_, N_), (L_, O_), (L_, N_)]
    assert per["l"][-1] == (L_, N_) and len(per["l"]) == 3 and per["m"][-1] == (L_, N_) and len(per["m"]) == 4
    assert per["n"] == per["l"] + [(N_, N_)] * 2 and per["o"][:4] == per["g"]
