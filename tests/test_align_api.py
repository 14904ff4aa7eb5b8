"""Nearest neighbours between two buffers, pair sums and the rigid fit, the parts that need no device: the
header declares the four entry points behind the stand-alone primitives with their notes, the ctypes layer binds them, the
Rust file and the C++ mirror name them, the Python layer refuses wrong arguments before any library call, gs_rigid_fit and
gs_model_transform_compose (host code) agree with numpy, and the restatement of tests/align_np.py agrees with a plain loop
and with the properties the GPU test relies on."""
import ctypes as C
import inspect
import math
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import align_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("gs_gaussians_buffer_knn_between", "gs_gaussians_buffer_pair_sums", "gs_rigid_fit", "gs_model_transform_compose")
TITLE = "Nearest neighbours between two buffers: rows, overlap select, rigid fit"
f32, u32 = np.float32, np.uint32


def test_header_declares_the_align_api(gs):
    text = open(os.path.join(ROOT, "include", "gs3d.h")).read()
    lib = gs._capi.load()
    vp, i32, c_u32, c_f32 = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
    want = {"gs_gaussians_buffer_knn_between": (i32, [vp, vp, vp, vp, vp, vp, vp, c_u32, c_f32, vp, vp]),
            "gs_gaussians_buffer_pair_sums": (i32, [vp, vp, vp, vp, vp, vp, vp, c_u32, vp]),
            "gs_rigid_fit": (i32, [vp, i32, vp, vp]),
            "gs_model_transform_compose": (None, [vp, vp, vp])}
    for entry in ENTRIES:
        assert hasattr(lib, entry), "the symbol is exported"
        assert gs._capi.SIGNATURES[entry] == want[entry]
        assert getattr(lib, entry).argtypes == want[entry][1] and getattr(lib, entry).restype == want[entry][0]
    assert text.count(TITLE) == 1
    # behind the stand-alone primitives: the slices of the earlier sections end there
    assert text.index("Stand-alone device primitives") < text.index("gs_exclusive_scan_u32(") < text.index(TITLE) < text.index("#ifdef __cplusplus\n}")
    section = text[text.index(TITLE):]
    comments = re.findall(r"/\*.*?\*/", section, flags=re.S)
    blocks = [c for c in comments if len(c) > 120]
    assert len(blocks) >= 5
    for c in blocks:
        assert "DESIGN.md 3.19" in c and "no reference item" in c, c[:80]
    for entry in ENTRIES:
        assert section.count(entry + "(") == 1
    assert "typedef struct gs_pair_sums" in section
    # the record: 152 bytes, the layout of the header
    rec = gs._capi.PairSumsRecord
    assert C.sizeof(rec) == 152 and [(n, getattr(rec, n).offset) for n, _ in rec._fields_] == [
        ("pairs", 0), ("sp", 8), ("sq", 32), ("spq", 56), ("spp", 128), ("sqq", 136), ("sdd", 144)]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**3.19 " in design and all(e in design for e in ENTRIES)
    assert "gs_align.hip" in design and "gs_align.hip" in open(os.path.join(ROOT, "README.md")).read()
    assert '"gs_align.hip"' in open(os.path.join(ROOT, "wgpu-3dgs-core_amd", "build.py")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "align_device_code.txt"))


def test_rust_and_cpp_name_the_align_api():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for entry in ENTRIES:
        assert "pub fn %s(" % entry in rs and entry + "(" in hpp
    decl = rs[rs.index("pub fn gs_gaussians_buffer_knn_between("):].split(";", 1)[0]
    assert "target: *mut gs_gaussians_buffer" in decl and "k: u32, radius: f32" in decl and "index_out: *mut gs_buffer" in decl
    decl = rs[rs.index("pub fn gs_gaussians_buffer_pair_sums("):].split(";", 1)[0]
    assert "index_plane: *const gs_buffer" in decl and "out: *mut gs_pair_sums" in decl
    assert "pub struct gs_pair_sums {" in rs and "pub spq: [f64; 9]," in rs
    assert "void knn_to(Stream &s, GaussiansBuffer<T> &target, uint32_t k, float radius" in hpp
    assert "gs_pair_sums pair_sums(Stream &s, GaussiansBuffer<T> &target" in hpp
    assert "inline gs_model_transform_pod rigid_fit(const gs_pair_sums &sums" in hpp
    assert "inline gs_model_transform_pod compose(const gs_model_transform_pod &delta" in hpp


def _stand_in(cls, **attrs):
    """a handle-less object: nothing it is given to may reach the library"""
    o = object.__new__(cls)
    o._h = None
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_align_arguments_are_checked_without_a_device(gs):
    buf = _stand_in(gs.GaussiansBuffer, pod=gs.GaussianPod(0, 0), device=None)
    other = _stand_in(gs.GaussiansBuffer, pod=gs.GaussianPod(0, 0), device=None)
    sel, plane = _stand_in(gs.Selection, device=None), _stand_in(gs.Buffer, device=None)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError):
            buf.knn_to(None, other, bad, 1.0)
        with pytest.raises(ValueError):
            buf.pair_sums(None, other, plane, bad)
    for bad in ("3", None, True, 3.0):
        with pytest.raises(TypeError):
            buf.knn_to(None, other, bad, 1.0)
    for bad in (-1.0, float("nan"), float("inf"), 1e20):          # 1e20 squared is not finite in binary32
        with pytest.raises(ValueError):
            buf.knn_to(None, other, 3, bad)
        with pytest.raises(ValueError):
            sel.select_near(_stand_in(gs.Stream), buf, other, bad)
        with pytest.raises(ValueError):
            buf.chamfer_to(_stand_in(gs.Stream), other, bad)
        with pytest.raises(ValueError):
            buf.align_to(_stand_in(gs.Stream), other, bad)
    with pytest.raises(TypeError):
        buf.knn_to(None, other, 3, "1")
    with pytest.raises(TypeError):
        buf.knn_to(None, np.zeros(4), 3, 1.0)
    with pytest.raises(ValueError):
        buf.knn_to(None, buf, 3, 1.0)                              # the buffer itself: that is knn()
    for kw in (dict(among=np.zeros(4, bool)), dict(queries=np.zeros(4, bool)), dict(model_transform=(0, 0, 0)),
               dict(target_transform=(0, 0, 0)), dict(dist2_out=np.zeros(12, f32)), dict(index_out=np.zeros(12, u32)), dict(indices=1)):
        with pytest.raises(TypeError):
            buf.knn_to(None, other, 3, 1.0, **kw)
    with pytest.raises(TypeError):
        buf.pair_sums(None, other, np.zeros(4, u32))
    with pytest.raises(TypeError):
        buf.pair_sums(None, plane, plane)
    with pytest.raises(TypeError):
        buf.pair_sums(None, other, plane, queries=np.zeros(4, bool))
    # the policies need a stream: they block on it
    for call in (lambda: buf.chamfer_to(None, other, 1.0), lambda: buf.align_to(None, other, 1.0), lambda: sel.select_near(None, buf, other, 1.0)):
        with pytest.raises(TypeError):
            call()
    st = _stand_in(gs.Stream)
    with pytest.raises(TypeError):
        sel.select_near(st, plane, other, 1.0)
    with pytest.raises(ValueError):
        sel.select_near(st, buf, other, 1.0, op="nand")
    with pytest.raises(ValueError):
        sel.select_near(st, buf, buf, 1.0)
    for kw, exc in ((dict(scale=1), TypeError), (dict(max_iterations=0), ValueError), (dict(max_iterations=2.0), TypeError),
                    (dict(rms_tol="1"), TypeError), (dict(rms_tol=-1.0), ValueError), (dict(rms_tol=float("nan")), ValueError),
                    (dict(queries=np.zeros(4, bool)), TypeError), (dict(model_transform=(0, 0, 0)), TypeError)):
        with pytest.raises(exc):
            buf.align_to(st, other, 1.0, **kw)
    with pytest.raises(TypeError):
        gs.rigid_fit(np.zeros(19))
    with pytest.raises(TypeError):
        gs.rigid_fit(gs.PairSums(3, np.zeros(3), np.zeros(3), np.zeros((3, 3)), 0.0, 0.0, 0.0), scale=1)
    with pytest.raises(TypeError):
        gs.compose_model_transform((0, 0, 0), gs.model_transform_pod())
    p = inspect.signature(gs.GaussiansBuffer.knn_to).parameters
    assert list(p)[1:] == ["stream", "target", "k", "radius", "queries", "among", "model_transform", "target_transform", "dist2_out",
                           "index_out", "indices"]
    assert all(p[n].default is None for n in list(p)[5:11]) and p["indices"].default is False
    p = inspect.signature(gs.GaussiansBuffer.align_to).parameters
    assert list(p)[1:] == ["stream", "target", "radius", "queries", "among", "model_transform", "target_transform", "scale",
                           "max_iterations", "rms_tol"]
    assert (p["scale"].default, p["max_iterations"].default) == (False, 32) and 0 < p["rms_tol"].default < 1
    assert list(inspect.signature(gs.GaussiansBuffer.chamfer_to).parameters)[1:4] == ["stream", "target", "radius"]
    assert list(inspect.signature(gs.Selection.select_near).parameters)[1:5] == ["stream", "gaussians", "target", "radius"]
    assert "gs_gaussians_buffer_knn_between" in gs.GaussiansBuffer.knn_to.__doc__
    assert "gs_gaussians_buffer_pair_sums" in gs.GaussiansBuffer.pair_sums.__doc__
    assert "gs_rigid_fit" in gs.rigid_fit.__doc__ and "gs_model_transform_compose" in gs.compose_model_transform.__doc__
    s = gs.PairSums(pairs=4, sp=np.zeros(3), sq=np.zeros(3), spq=np.zeros((3, 3)), spp=0.0, sqq=0.0, sdd=16.0)
    assert s.rms == 2.0 and C.sizeof(s.record()) == 152
    assert math.isnan(gs.PairSums(0, np.zeros(3), np.zeros(3), np.zeros((3, 3)), 0.0, 0.0, 0.0).rms)


def test_null_arguments_are_errors_of_the_c_abi(gs):
    """no device is touched"""
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    out = gs._capi.PairSumsRecord()
    out.pairs = 7
    pod = gs.model_transform_pod((1, 2, 3))
    assert lib.gs_gaussians_buffer_knn_between(None, None, None, None, None, None, None, 3, 1.0, None, None) == bad
    assert lib.gs_gaussians_buffer_pair_sums(None, None, None, None, None, None, None, 1, C.byref(out)) == bad and out.pairs == 7
    assert lib.gs_rigid_fit(None, 0, C.byref(pod), None) == bad and lib.gs_rigid_fit(C.byref(out), 0, None, None) == bad
    lib.gs_model_transform_compose(None, C.byref(pod), C.byref(pod))
    lib.gs_model_transform_compose(C.byref(pod), C.byref(pod), None)
    assert list(pod.pos) == [1.0, 2.0, 3.0]


# ---- the restatement against a plain loop ---------------------------------------------------------------------------------

def _r(x):
    """x rounded to binary32, as a Python float"""
    return struct.unpack("f", struct.pack("f", x))[0]


def _bits(x):
    return struct.unpack("I", struct.pack("f", x))[0]


def _loop_rows(pq, pt, k, radius, queries, among):
    """the definition as a plain Python loop; every operation rounded to binary32 by a round trip through 4 bytes"""
    rr = _r(_r(radius) * _r(radius))
    tpoint = [bool(among[j]) and all(math.isfinite(c) for c in pt[j]) for j in range(len(pt))]
    d2_rows, ix_rows = [], []
    for i in range(len(pq)):
        if not queries[i] or not all(math.isfinite(c) for c in pq[i]):
            d2_rows.append([float("nan")] * k)
            ix_rows.append([align_np.NONE] * k)
            continue
        cand = []
        for j in range(len(pt)):
            if not tpoint[j]:
                continue
            d = [_r(float(pq[i][a]) - float(pt[j][a])) for a in range(3)]
            d2 = _r(_r(_r(d[0] * d[0]) + _r(d[1] * d[1])) + _r(d[2] * d[2]))
            if d2 <= rr:
                cand.append((_bits(d2), j, d2))
        cand.sort()
        cand = cand[:k]
        d2_rows.append([c[2] for c in cand] + [float("inf")] * (k - len(cand)))
        ix_rows.append([c[1] for c in cand] + [align_np.NONE] * (k - len(cand)))
    return np.array(d2_rows, f32).reshape(len(pq), k), np.array(ix_rows, u32).reshape(len(pq), k)


def _forty_fifty():
    rng = np.random.default_rng(41)
    pt = rng.uniform(-1, 1, (50, 3)).astype(f32)
    pq = rng.uniform(-1, 1, (40, 3)).astype(f32)
    pq[3] = pt[17]                           # cross-buffer duplicates: distance 0, and no self-exclusion
    pt[30:33] = pt[17]
    pq[21] = f32([5, 5, 5])                  # an exact tie at a distance, away from the others
    pt[9] = f32([5.25, 5, 5])
    pt[4] = f32([4.75, 5, 5])
    pq[7, 1] = np.nan
    pq[8, 0] = np.inf
    pt[11, 2] = np.nan
    pt[12, 0] = -np.inf
    among = np.ones(50, bool)
    among[[2, 31, 40]] = False
    queries = np.ones(40, bool)
    queries[[5, 21 + 1, 33]] = False
    return pq, pt, queries, among


def test_restatement_equals_a_plain_loop():
    pq, pt, queries, among = _forty_fifty()
    for k in (1, 3, 16):
        for radius in (0.0, 0.25, 0.6, 5.0):
            d2, ix, written = align_np.rows_between(pq, pt, k, radius, queries, among)
            ld2, lix = _loop_rows(pq, pt, k, radius, queries, among)
            assert np.array_equal(d2.view(u32), ld2.view(u32)) and np.array_equal(ix, lix), (k, radius)
            assert np.array_equal(written, queries)
            assert np.isnan(d2[[5, 7, 8, 22, 33]]).all() and not np.isnan(d2[[0, 3, 21]]).any()
            assert not np.isin(ix, [2, 11, 12, 31, 40]).any()
    d2, ix, _ = align_np.rows_between(pq, pt, 3, 0.0, queries, among)
    assert np.array_equal(ix[3], [17, 30, 32]) and (d2[3].view(u32) == 0).all()      # 31 is outside `among`
    d2, ix, _ = align_np.rows_between(pq, pt, 2, 0.25, queries, among)
    assert np.array_equal(ix[21], [4, 9]) and d2[21, 0] == d2[21, 1]                  # the tie goes to the smaller target index
    # a complete row is the same at every larger radius, and the row of k is the first k entries of the row of 16
    d16, i16, _ = align_np.rows_between(pq, pt, 16, 0.6, queries, among)
    for k in (1, 3, 8):
        a, ai, _ = align_np.rows_between(pq, pt, k, 0.6, queries, among)
        b, bi, _ = align_np.rows_between(pq, pt, k, 1.2, queries, among)
        complete = np.isfinite(a[:, -1])
        assert complete.any() and np.array_equal(a[complete].view(u32), b[complete].view(u32)) and np.array_equal(ai[complete], bi[complete])
        assert np.array_equal(a.view(u32), d16[:, :k].view(u32)) and np.array_equal(ai, i16[:, :k])
    # the pair sums: an index at or beyond the target's length, a NaN on either side and a hole of `queries` form no pair
    first = align_np.rows_between(pq, pt, 1, 5.0, None, None)[1][:, 0]
    s = align_np.pair_sums(pq, pt, first, queries)
    ok, terms = align_np.pair_terms(pq, pt, first, queries)
    assert s["pairs"] == ok.sum() == 40 - 2 - 3 and not ok[[5, 7, 8, 22, 33]].any()
    assert terms.shape == (35, 18) and s["sums"][17] == pytest.approx(float((terms[:, 17]).sum()), rel=1e-14)
    assert align_np.pair_sums(pq, pt, np.full(40, 50, u32))["pairs"] == 0 and align_np.pair_sums(pq, pt, np.full(40, align_np.NONE, u32))["pairs"] == 0


# ---- gs_rigid_fit and gs_model_transform_compose against numpy -------------------------------------------------------------

def _sums_of(gs, p, q):
    """the PairSums of the pairs (p_i, q_i), float32 positions, by the restatement"""
    s = align_np.pair_sums(p, q, np.arange(len(p), dtype=u32))
    v = s["sums"]
    return s, gs.PairSums(pairs=s["pairs"], sp=v[0:3], sq=v[3:6], spq=v[6:15].reshape(3, 3), spp=v[15], sqq=v[16], sdd=v[17])


def _fit_cases():
    rng = np.random.default_rng(7)
    out = []
    for n, noise, scale in ((60, 0.0, 1.0), (60, 0.02, 1.0), (200, 0.05, 1.7), (12, 0.0, 0.6)):
        p = rng.uniform(-2, 2, (n, 3))
        q4 = rng.normal(size=4)
        q4 /= np.linalg.norm(q4)
        R = align_np.quat_matrix(q4)
        q = scale * p @ R.T + rng.uniform(-1, 1, 3) + noise * rng.normal(size=(n, 3))
        out.append((p.astype(f32), q.astype(f32), scale != 1.0))
    return out


def test_rigid_fit_equals_the_numpy_fit(gs):
    for p, q, with_scale in _fit_cases():
        s, sums = _sums_of(gs, p, q)
        want = align_np.rigid_fit(s["pairs"], s["sums"], with_scale)
        gap = want["eig"][-1] - want["eig"][-2]
        assert gap / want["fro"] >= 0.1, "the input determines its rotation well"
        bound = 64 * 2.0 ** -52 * want["fro"] / gap
        delta, rms = gs.rigid_fit(sums, scale=with_scale)
        got = np.array([delta.rot[3], delta.rot[0], delta.rot[1], delta.rot[2]], np.float64)
        assert got[0] >= 0
        if got @ want["quat"] < 0:      # (w = 0: the sign is the first component's)
            got = -got
        # the pod holds the quaternion in binary32: a value within `bound` of the reference, correctly rounded, lies within
        # the bound plus half the binary32 spacing at that component
        err = np.abs(got - want["quat"])
        half_ulp = 0.5 * np.spacing((np.abs(want["quat"]) + bound).astype(f32)).astype(np.float64)
        print("rigid_fit: n %d, gap / |N| %.3f, quaternion error %.3g, bound %.3g + half a binary32 step (%.3g at the largest)" %
              (len(p), gap / want["fro"], err.max(), bound, half_ulp.max()))
        assert (err <= bound + half_ulp).all(), (err, bound, half_ulp)
        assert rms == want["rms"] or abs(rms - want["rms"]) <= 2.0 ** -52 * want["rms"]
        assert np.allclose(list(delta.scale), want["scale"], rtol=2.0 ** -22, atol=0) and delta.scale[0] == delta.scale[1] == delta.scale[2]
        assert np.allclose(list(delta.pos), want["t"], rtol=0, atol=2.0 ** -21 * (1 + np.abs(want["t"]).max() + np.abs(s["sums"][0:6]).max() / len(p)))
        if not with_scale:
            assert delta.scale[0] == 1.0
            # ... and Horn's quaternion is the rotation of the SVD solution
            assert np.allclose(want["R"], align_np.rigid_fit_svd(p, q), atol=1e-9)


def test_rigid_fit_refuses_what_determines_no_transform(gs):
    p, q, _ = _fit_cases()[0]
    _, good = _sums_of(gs, p, q)
    gs.rigid_fit(good)
    bad = gs.InvalidArgumentError
    _, two = _sums_of(gs, p[:2], q[:2])
    with pytest.raises(bad):
        gs.rigid_fit(two)
    # collinear p: a rotation about the line is free
    line = np.outer(np.arange(6, dtype=np.float64), [1.0, 2.0, -0.5]).astype(f32)
    _, sums = _sums_of(gs, line, (line + f32([1, 0, 2])).astype(f32))
    for with_scale in (True, False):
        with pytest.raises(bad):
            gs.rigid_fit(sums, scale=with_scale)
    # no spread: every p is one point
    _, sums = _sums_of(gs, np.tile(p[:1], (5, 1)), q[:5])
    with pytest.raises(bad):
        gs.rigid_fit(sums, scale=True)
    for field in ("sp", "spq", "sdd"):
        _, sums = _sums_of(gs, p, q)
        if field == "sdd":
            sums.sdd = float("nan")
        else:
            getattr(sums, field).reshape(-1)[1] = float("nan") if field == "sp" else float("inf")
        with pytest.raises(bad):
            gs.rigid_fit(sums)
    # the outputs are untouched on error
    lib = gs._capi.load()
    pod, rms = gs.model_transform_pod((1, 2, 3)), C.c_double(5.0)
    rec = two.record()
    assert lib.gs_rigid_fit(C.byref(rec), 0, C.byref(pod), C.byref(rms)) == bad.code and list(pod.pos) == [1.0, 2.0, 3.0] and rms.value == 5.0


def test_compose_equals_the_matrix_product(gs):
    rng = np.random.default_rng(3)
    for case in range(6):
        dq, mq = rng.normal(size=4), rng.normal(size=4)
        dq, mq = dq / np.linalg.norm(dq), mq / np.linalg.norm(mq)
        sd = float(rng.uniform(0.5, 2.0)) if case % 2 else 1.0
        delta = gs.model_transform_pod(tuple(rng.uniform(-3, 3, 3)), tuple(dq), (sd, sd, sd))
        m = gs.model_transform_pod(tuple(rng.uniform(-3, 3, 3)), tuple(mq), (1.25, 0.75, 2.0) if case >= 2 else (1.0, 1.0, 1.0))
        out = gs.compose_model_transform(delta, m)
        pods = [(list(x.pos), list(x.rot), list(x.scale)) for x in (delta, m, out)]
        want = align_np.pod_matrix(*pods[0]) @ align_np.pod_matrix(*pods[1])
        assert np.allclose(align_np.pod_matrix(*pods[2]), want, rtol=0, atol=2.0 ** -20 * np.abs(want).max())
        pos, rot, scale = align_np.compose(pods[0], pods[1])
        assert np.array_equal(f32(pos), f32(pods[2][0])) and np.array_equal(f32(rot), f32(pods[2][1])) and np.array_equal(f32(scale), f32(pods[2][2]))
    ident = gs.model_transform_pod()
    out = gs.compose_model_transform(ident, m)
    assert bytes(out) == bytes(m)


# ---- the ICP input of the GPU test ------------------------------------------------------------------------------------------

def test_one_iteration_is_exact_on_the_icp_input(gs):
    case = align_np.icp_case()
    target, query, mate = case["target"], case["query"], case["mate"]
    assert len(target) == 729 and len(query) == int(0.4 * 729) and len(np.unique(mate)) == len(mate)
    disp = np.linalg.norm(query.astype(np.float64) - target[mate].astype(np.float64), axis=1)
    print("ICP input: displacement max %.4f, mean %.4f" % (disp.max(), disp.mean()))
    assert 0.05 < disp.max() <= 0.3
    # neighbours in the target are at least 0.8 apart, so a query within 0.3 of its mate is more than 0.5 from every other
    d2, ix, _ = align_np.rows_between(query, target, 2, 0.45)
    assert np.array_equal(ix[:, 0], mate) and (ix[:, 1] == align_np.NONE).all()
    s, sums = _sums_of(gs, query, target[mate])
    delta, rms = gs.rigid_fit(sums)
    assert rms == pytest.approx(math.sqrt(float((disp * disp).mean())), rel=1e-12)
    R = align_np.quat_matrix((delta.rot[3], delta.rot[0], delta.rot[1], delta.rot[2]))
    moved = query.astype(np.float64) @ R.T + np.array(list(delta.pos), np.float64)
    left = np.linalg.norm(moved - target[mate].astype(np.float64), axis=1)
    assert left.max() < 1e-5 and np.allclose(R, case["R"], atol=1e-6) and np.allclose(list(delta.pos), case["t"], atol=1e-5)
