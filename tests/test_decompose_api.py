"""Covariance -> rotation + scale, the parts that need no device: the exact cases of the definition, the host
function gs_cov3d_decompose against a float64 witness (tests/decompose_np.py) over the set, the record function
gs_decompose_pods against gs_convert_pods and gs_cov3d_decompose, its errors, the header / bindings / docstrings, and the
picture of host-decomposed records through the oracle."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import decompose_np as dn
from helpers import bits, default_camera, same_bits
from scenes import ALL_LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gs_cov3d_decompose", "gs_decompose_pods", "gs_gaussians_buffer_create_decomposed"]
f32 = np.float32
IDENTITY = np.array([0, 0, 0, 1], f32)
SH_BYTES, COV_BYTES = (180, 92, 48, 0), (28, 24, 12)
# The maxima of the two error measures over the set, measured once on the host function (NOTES.md "Covariance -> rotation +
# scale"): eigenvalues 3.0508e-07, reconstruction 7.4762e-07.  The bounds are 4 x those (head room for the quaternion
# conversion); both stay below 1e-5.
EIGENVALUE_BOUND = 4 * 3.0508e-07
RECONSTRUCTION_BOUND = 4 * 7.4762e-07


@pytest.fixture(scope="module")
def the_set(gs):
    return dn.the_set(gs)


@pytest.fixture(scope="module")
def decomposed(gs, the_set):
    """{"f32" / "f16": (rot, scale) of the set's covariances by the host function}: once, read-only"""
    out = {}
    for name in ("f32", "f16"):
        q, s = dn.decompose_many(gs, the_set[name])
        q.setflags(write=False)
        s.setflags(write=False)
        out[name] = (q, s)
    return out


# ---- exact cases -----------------------------------------------------------------------------------------------------

def test_diagonal_zero_and_isotropic_inputs(gs):
    rng = np.random.default_rng(1)
    for d in list(np.exp(rng.uniform(np.log(1e-15), np.log(1e15), (200, 3))).astype(f32)) + [f32([4, 1, 0]), f32([0, 0, 2.5]),
                                                                                             f32([1e-42, 3e-45, 0])]:
        q, s = gs.cov3d_decompose([d[0], 0, 0, d[1], 0, d[2]])
        assert same_bits(q, IDENTITY) and same_bits(s, np.sqrt(d)), (d, q, s)
    for z in ([0.0] * 6, [-0.0] * 6, [0.0, -0.0, 0.0, -0.0, 0.0, -0.0]):
        q, s = gs.cov3d_decompose(z)
        assert same_bits(q, IDENTITY) and same_bits(s, np.zeros(3, f32)), z
    for c in np.exp(rng.uniform(np.log(1e-38), np.log(1e38), 200)).astype(f32):
        q, s = gs.cov3d_decompose([c, 0, 0, c, 0, c])
        assert same_bits(q, IDENTITY) and same_bits(s, np.full(3, np.sqrt(c), f32)), c


def test_non_finite_words(gs):
    base = f32([2.0, 0.25, -0.5, 3.0, 0.125, 1.5])
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            c = base.copy()
            c[k] = bad
            q, s = gs.cov3d_decompose(c)
            assert same_bits(q, IDENTITY) and (bits(s) == 0x7FC00000).all(), (k, bad, q, s)


def test_scale_invariance(gs, the_set):
    """decompose(4^k C): the same rotation bits, the scales exactly 2^k times those of decompose(C)"""
    c = np.concatenate([the_set["f32"][:800], the_set["f32"][-200:]])
    q0, s0 = dn.decompose_many(gs, c)
    for k in (-20, -2, 2, 20):
        ck = c * f32(4.0) ** k
        assert np.array_equal(ck.astype(np.float64), c.astype(np.float64) * 4.0 ** k)      # the scaling itself is exact
        q, s = dn.decompose_many(gs, ck)
        assert same_bits(q, q0), k
        assert same_bits(s, s0 * f32(2.0) ** k), k


# ---- against the witness ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["f32", "f16"])
def test_unit_quaternion(decomposed, name):
    q, s = decomposed[name]
    assert np.isfinite(q).all() and np.isfinite(s).all() and (s >= 0).all()
    assert np.abs((q.astype(np.float64) ** 2).sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -23
    assert (q[:, 3] >= 0).all()


@pytest.mark.parametrize("name", ["f32", "f16"])
def test_eigenvalues_against_the_witness(the_set, decomposed, name):
    err = dn.eigenvalue_error(decomposed[name][1], the_set[name]).max()
    print("eigenvalue error over the %s set: %.4e (bound %.4e)" % (name, err, EIGENVALUE_BOUND))
    assert EIGENVALUE_BOUND <= 1e-5 and err <= EIGENVALUE_BOUND


@pytest.mark.parametrize("name", ["f32", "f16"])
def test_reconstruction_against_the_witness(gs, the_set, decomposed, name):
    q, s = decomposed[name]
    err = dn.reconstruction_error(dn.repack_cov(gs, q, s), the_set[name]).max()
    print("reconstruction error over the %s set: %.4e (bound %.4e)" % (name, err, RECONSTRUCTION_BOUND))
    assert RECONSTRUCTION_BOUND <= 1e-5 and err <= RECONSTRUCTION_BOUND


def test_a_zero_covariance_of_the_set_gives_zero_scales(the_set, decomposed):
    """f16 flushes the smallest covariances of the set to zero: the relative measures above say nothing about them"""
    zero = np.abs(the_set["f16"]).max(axis=1) == 0
    q, s = decomposed["f16"]
    assert zero.any() and same_bits(s[zero], np.zeros_like(s[zero])) and same_bits(q[zero], np.tile(IDENTITY, (zero.sum(), 1)))


# ---- records ---------------------------------------------------------------------------------------------------------

N = 257


@pytest.fixture(scope="module")
def packed(gs):
    g = dn.set_gaussians(N, seed=21)
    out = {l: gs.GaussianPod(*l).from_gaussian(g) for l in ALL_LAYOUTS}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("ssh", range(4))
def test_a_rot_scale_source_is_the_conversion(gs, packed, ssh):
    src = gs.GaussianPod(ssh, 0)
    for dsh in range(4):
        got, want = src.decompose(packed[(ssh, 0)], dsh), src.convert(packed[(ssh, 0)], gs.GaussianPod(dsh, 0))
        assert np.array_equal(got, want), (ssh, dsh)


@pytest.mark.parametrize("src", [l for l in ALL_LAYOUTS if l[1] != 0])
def test_records_of_a_covariance_source(gs, packed, src):
    spod = gs.GaussianPod(*src)
    c6 = dn.cov_words(gs, packed[src], *src)
    q, s = gs.cov3d_decompose(c6)
    for dsh in range(4):
        dpod = gs.GaussianPod(dsh, 0)
        got = spod.decompose(packed[src], dsh).reshape(N, -1)
        assert got.shape[1] == dpod.size
        head = 16 + SH_BYTES[dsh]
        same_cov = spod.convert(packed[src], gs.GaussianPod(dsh, src[1])).reshape(N, -1)
        assert np.array_equal(got[:, :head], same_cov[:, :head]), (src, dsh)                # words 0..3 and the SH section
        assert same_bits(got[:, head:head + 16], q) and same_bits(got[:, head + 16:head + 28], s), (src, dsh)
        assert not got[:, head + 28:].any(), (src, dsh)                                        # the trailing pad


def test_errors_are_those_of_the_conversion(gs):
    lib = gs._capi.load()
    bad = gs.InvalidArgumentError.code
    buf = np.full(256, 0xAB, np.uint8)
    src = np.zeros(256, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for cov in range(3):
        assert lib.gs_decompose_pods(0, cov, 1, None, 1, p(buf)) == bad == lib.gs_convert_pods(0, cov, 1, cov, None, 1, p(buf))
        assert lib.gs_decompose_pods(0, cov, 1, p(src), 1, None) == bad == lib.gs_convert_pods(0, cov, 1, cov, p(src), 1, None)
        for cfg in ((4, cov, 1), (-1, cov, 1), (0, cov, 4), (0, cov, -1), (0, 3, 1)):
            assert lib.gs_decompose_pods(*cfg, p(src), 1, p(buf)) == bad, cfg
    assert (buf == 0xAB).all()
    # every known combination is defined
    for ssh, scov in ALL_LAYOUTS:
        for dsh in range(4):
            assert lib.gs_decompose_pods(ssh, scov, dsh, p(src), 1, p(buf)) == 0, (ssh, scov, dsh)
    pod = gs.GaussianPod(1, 2)
    with pytest.raises(ValueError):
        pod.decompose(np.zeros(pod.size + 1, np.uint8), 0)
    assert pod.decompose(np.zeros(0, np.uint8), 0).size == 0


def test_the_pair_table_is_unchanged(gs):
    lib = gs._capi.load()
    pairs = [(a, b) for a in ALL_LAYOUTS for b in ALL_LAYOUTS]
    assert sum(lib.gs_layout_convertible(*a, *b) for a, b in pairs) == 112
    src, out = np.zeros(224, np.uint8), np.full(224, 0xAB, np.uint8)
    rc = lib.gs_convert_pods(1, 2, 1, 0, src.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p))
    assert rc == gs.LossyConfigError.code and (out == 0xAB).all()


# ---- header, bindings, documents -------------------------------------------------------------------------------------

def test_header_bindings_and_docstrings_name_the_entry_points(gs):
    text = open(os.path.join(ROOT, "include", "gs3d.h")).read()
    lib = gs._capi.load()
    section = text[text.index("Layout conversion"):text.index("Stand-alone device primitives")]
    for name in ENTRIES:
        assert name in gs._capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == gs._capi.SIGNATURES[name][1]
        assert len(re.findall(r"\b%s\s*\(" % name, text)) == 1, name
        comment = section[:section.index(name + "(")].rsplit("/*", 1)[1]
        assert "no reference item" in comment and "DESIGN.md 3.12a" in comment, name
    assert re.search(r"#define\s+GS3D_ABI_VERSION\s+1\b", text) and lib.gs_abi_version() == 1
    hpp = open(os.path.join(ROOT, "include", "gs3d.hpp")).read()
    for name in ENTRIES:
        assert name in hpp, name
    assert "gs_decompose_pods" in gs.GaussianPod.decompose.__doc__
    assert "gs_gaussians_buffer_create_decomposed" in gs.GaussiansBuffer.decompose.__doc__
    assert "gs_cov3d_decompose" in gs.cov3d_decompose.__doc__
    for method in (gs.GaussiansBuffer.write, gs.GaussiansBuffer.export_ply, gs.GaussiansBuffer.export_spz,
                   gs.GaussiansBuffer.export_spz_file):
        assert "decompose" in method.__doc__, method
    assert "**3.12a " in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_rust_bindings_are_in_sync():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    rs = open(os.path.join(ROOT, "bindings", "rust", "gs3d_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn %s\(" % name, rs), name


def test_python_layer_checks_arguments_without_a_device(gs):
    buf = object.__new__(gs.GaussiansBuffer)
    buf._h, buf.pod = None, gs.GaussianPod(1, 2)
    with pytest.raises(TypeError):
        buf.decompose(None, 1, selection=np.zeros(4, bool))
    with pytest.raises(ValueError):
        gs.cov3d_decompose(np.zeros(5, f32))


# ---- picture ---------------------------------------------------------------------------------------------------------

def test_the_picture_of_decomposed_records(gs, ob):
    """E_impl <= 4 E_wit + 1e-4: the frame of the host-decomposed records is as close to the frame of the cov-f32 records they
    came from as the frame of records decomposed in float64 (1e-4: the per-channel frame tolerance; 4: tile-rect differences
    of single splats)"""
    import synth
    n, W, H = 2000, 64, 64
    g = synth.scene(n, first=5)
    src = gs.GaussianPod(0, 1)
    pods = src.from_gaussian(g)
    ogt, omt, ocam = ob.gaussian_transform(sh_deg=3), ob.model_transform(), default_camera(ob, W, H)
    order = np.arange(n, dtype=np.uint32)
    want, _, vis, _ = ob.render(0, 1, pods, ogt, omt, ocam, order=order)
    assert vis > 100
    impl = src.decompose(pods, 0)
    lam, v, _, _ = dn.witness(dn.cov_words(gs, pods, 0, 1))
    wit = impl.reshape(n, -1).copy()
    wit[:, 196:212] = dn.quaternion(v).astype(f32).view(np.uint8)
    wit[:, 212:224] = np.sqrt(lam).astype(f32).view(np.uint8)
    e_impl = np.abs(ob.render(0, 0, impl, ogt, omt, ocam, order=order)[0] - want).mean()
    e_wit = np.abs(ob.render(0, 0, wit.reshape(-1), ogt, omt, ocam, order=order)[0] - want).mean()
    print("picture: E_impl %.4e E_wit %.4e" % (e_impl, e_wit))
    assert e_impl <= 4 * e_wit + 1e-4
