"""wgpu_3dgs_core_amd — host-side mirror of LioQing/wgpu-3dgs-core's API over the MI355X C ABI.

The product is libgs3d_hip.so (include/gs3d.h); this package is the thin Python host layer that
tests, bench.py and torch.distributed plumbing use.  Names, argument meaning and error behaviour
follow the reference (citations relative to the reference repository):

    Gaussian / GaussianPod configs ...... src/gaussian.rs:53-60, src/buffer/gaussian.rs:239-384
    GaussiansBuffer ..................... src/buffer/gaussian.rs:17-229
    GaussianTransformBuffer / Pod ....... src/buffer/gaussian_transform.rs
    ModelTransformBuffer / Pod .......... src/buffer/model_transform.rs
    BufferWrapper.download .............. src/buffer/mod.rs:17-102
    ComputeBundle / ComputeBundleBuilder  src/compute_bundle.rs
    error enums ......................... src/error.rs:55-143

There is no CPU implementation behind any device call: constructing a Device without a HIP GPU
raises NoDeviceError, and importing the package without libgs3d_hip.so raises ImportError.
"""
import ctypes as C
import dataclasses

import numpy as np

from . import _capi
from ._capi import AttributeDesc, AuxTargets, Camera, Edit, FrameResult, FrameSelection, FrameStats, GaussianTransformPod, Limits, ModelTransformPod, SortInfo

_L = _capi.load()

# ------------------------------------------------------------------------------------------------
# data model
# ------------------------------------------------------------------------------------------------

#: struct Gaussian — src/gaussian.rs:53-60
GAUSSIAN_DTYPE = np.dtype([("rot", "<f4", 4), ("pos", "<f4", 3), ("color", "u1", 4),
                           ("sh", "<f4", 45), ("scale", "<f4", 3)])
#: projected splat record (include/gs3d.h gs_projected)
PROJECTED_DTYPE = np.dtype([("mx", "<f4"), ("my", "<f4"), ("ca", "<f4"), ("cb", "<f4"),
                            ("cc", "<f4"), ("opacity", "<f4"), ("r", "<f4"), ("g", "<f4"),
                            ("b", "<f4"), ("depth", "<f4"), ("tx0", "<u2"), ("ty0", "<u2"),
                            ("tx1", "<u2"), ("ty1", "<u2")])

SH_SINGLE, SH_HALF, SH_NORM8, SH_NONE = 0, 1, 2, 3
COV3D_ROT_SCALE, COV3D_SINGLE, COV3D_HALF = 0, 1, 2
SH_CONFIG_NAMES = ["Single", "Half", "Norm8", "None"]
COV3D_CONFIG_NAMES = ["RotScale", "Single", "Half"]
FEATURE_NAMES = [_L.gs_feature_name(i).decode() for i in range(7)]

DISPLAY_SPLAT, DISPLAY_ELLIPSE, DISPLAY_POINT = 0, 1, 2

KERNEL_ARRAY_MAP_ADD = 0
KERNEL_TEST_GAUSSIAN = 1
KERNEL_TEST_GAUSSIAN_TRANSFORM = 2
KERNEL_TEST_MODEL_TRANSFORM = 3
KERNEL_UNPACK_SOA = 4


class GsError(Exception):
    """Base of every error raised by the C ABI; carries the variant fields of src/error.rs."""
    code = None

    def __init__(self, info):
        self.status = info.code
        self.a, self.b, self.c = info.a, info.b, info.c
        super().__init__(info.message.decode(errors="replace"))


class InvalidArgumentError(GsError): code = -1
class NoDeviceError(GsError): code = -2
class HipError(GsError): code = -3
class OutOfMemoryError(GsError): code = -4


class GaussiansBufferUpdateError(GsError):
    """CountMismatch{count, expected_count} — src/error.rs:66-70"""
    code = -10
    count = property(lambda s: s.a)
    expected_count = property(lambda s: s.b)


class GaussiansBufferUpdateRangeError(GsError):
    """CountMismatch{count, start, expected_count} — src/error.rs:73-81"""
    code = -11
    count = property(lambda s: s.a)
    start = property(lambda s: s.b)
    expected_count = property(lambda s: s.c)


class GaussiansBufferTryFromBufferError(GsError):
    """BufferSizeNotMultiple{buffer_size, expected_multiple_size} — src/error.rs:85-94"""
    code = -12
    buffer_size = property(lambda s: s.a)
    expected_multiple_size = property(lambda s: s.b)


class FixedSizeBufferWrapperError(GsError):
    """BufferSizeMismatched{buffer_size, expected_size} — src/error.rs:97-104"""
    code = -13
    buffer_size = property(lambda s: s.a)
    expected_size = property(lambda s: s.b)


class ComputeBundleCreateError(GsError):
    """ResourceCountMismatch / WorkgroupSizeExceedsDeviceLimit — src/error.rs:107-126"""


class ResourceCountMismatch(ComputeBundleCreateError):
    code = -14
    resource_count = property(lambda s: s.a)
    bind_group_layout_count = property(lambda s: s.b)


class WorkgroupSizeExceedsDeviceLimit(ComputeBundleCreateError):
    code = -15
    workgroup_size = property(lambda s: s.a)
    device_limit = property(lambda s: s.b)


class ComputeBundleBuildError(Exception):
    """src/error.rs:129-143; raised by ComputeBundleBuilder.build in the reference's order."""


class MissingBindGroupLayout(ComputeBundleBuildError): pass
class MissingResolver(ComputeBundleBuildError): pass
class MissingEntryPoint(ComputeBundleBuildError): pass
class MissingMainShader(ComputeBundleBuildError): pass
class KernelResolveError(ComputeBundleBuildError): """ComputeBundleBuildError::Wesl analogue"""


class LossyConfigError(GsError): code = -21
class SpzError(GsError):
    """std::io::Error of the SPZ reader / header validation"""
    code = -25


class PlyError(GsError):
    """std::io::Error of PlyGaussians::read_from (message = the reference's message)"""
    code = -24
class DownloadBufferError(GsError): code = -22
class PairOverflowError(GsError):
    """a frame needs more (tile, Gaussian) pairs than 32-bit pair indices can address"""
    code = -23


class PairCapacityError(GsError):
    """gs_renderer_wait_frame: the frame produced more pairs than the renderer's buffers hold and was
    SKIPPED (its image was not written).  The next frame grows the buffers: render again.
    A two-round frame bounds each round on its own: `pairs` is then the count of the round that outgrew
    the bound (round 1 if both did), `capacity` that bound, and the message names the round.  Skipped by
    round 1, the image was not written; skipped by round 2, the frame's band holds round 1's
    intermediate pixel state (a known defect, include/gs3d.h at gs_renderer_set_rounds): not a frame."""
    code = -26

    def __init__(self, info):
        super().__init__(info)
        self.pairs, self.capacity = info.a, info.b


class RankOrderError(GsError):
    """gs_renderer_wait_frame: the watchdog of the radix sort's LDS-atomic rank fired in this frame (its blend
    order may be wrong).  The device has been switched to the ballot-based rank: render again."""
    code = -27


_ERRORS = {c.code: c for c in (InvalidArgumentError, NoDeviceError, HipError, OutOfMemoryError,
                               GaussiansBufferUpdateError, GaussiansBufferUpdateRangeError,
                               GaussiansBufferTryFromBufferError, FixedSizeBufferWrapperError,
                               ResourceCountMismatch, WorkgroupSizeExceedsDeviceLimit,
                               LossyConfigError, DownloadBufferError, PlyError, SpzError, PairOverflowError,
                               PairCapacityError, RankOrderError)}


def _check(status):
    if status == 0:
        return
    info = _capi.ErrorInfo()
    _L.gs_last_error(C.byref(info))
    if info.code != status:
        info.code = status
        info.message = _L.gs_status_string(status)
    raise _ERRORS.get(status, GsError)(info)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class GaussianPod:
    """One of the 12 GaussianPodWithSh{S}Cov3d{C}Configs layouts (src/buffer/gaussian.rs:373-384)."""

    def __init__(self, sh, cov):
        self.sh, self.cov = int(sh), int(cov)
        self.name = "GaussianPodWithSh%sCov3d%sConfigs" % (SH_CONFIG_NAMES[sh], COV3D_CONFIG_NAMES[cov])

    @property
    def size(self):
        return _L.gs_pod_size(self.sh, self.cov)

    def features(self):
        """GaussianPod::features() — src/buffer/gaussian.rs:270-286"""
        out = (C.c_uint8 * 7)()
        _check(_L.gs_pod_features(self.sh, self.cov, out))
        return [(FEATURE_NAMES[i], bool(out[i])) for i in range(7)]

    def from_gaussian(self, gaussians):
        """G::from_gaussian over an array of Gaussians -> packed bytes (host)."""
        g = np.ascontiguousarray(np.atleast_1d(gaussians), dtype=GAUSSIAN_DTYPE)
        out = np.zeros(len(g) * self.size, dtype=np.uint8)
        _check(_L.gs_pack(self.sh, self.cov, _ptr(g), len(g), _ptr(out)))
        return out

    def into_gaussian(self, pods):
        """Into<Gaussian>; raises LossyConfigError where the reference panics."""
        pods = np.ascontiguousarray(pods, dtype=np.uint8)
        n = len(pods) // self.size
        out = np.zeros(n, dtype=GAUSSIAN_DTYPE)
        _check(_L.gs_unpack_to_gaussian(self.sh, self.cov, _ptr(pods), n, _ptr(out)))
        return out

    def convertible_to(self, other):
        """gs_layout_convertible: can records of this layout be converted to `other`?  Every pair but
        those that would turn a covariance back into rotation and scale."""
        if not isinstance(other, GaussianPod):
            raise TypeError("other must be a GaussianPod, not %s" % type(other).__name__)
        return bool(_L.gs_layout_convertible(self.sh, self.cov, other.sh, other.cov))

    def convert(self, pods, to):
        """gs_convert_pods: packed records of this layout -> packed records of layout `to`, on the host,
        with the per-record function the device kernel calls.  Raises LossyConfigError for a pair that is not defined."""
        if not isinstance(to, GaussianPod):
            raise TypeError("to must be a GaussianPod, not %s" % type(to).__name__)
        pods = np.ascontiguousarray(pods, dtype=np.uint8).reshape(-1)
        if pods.size % self.size:
            raise ValueError("%d bytes are no whole number of %d-byte records" % (pods.size, self.size))
        n = pods.size // self.size
        out = np.zeros(max(n * to.size, 1), dtype=np.uint8)
        _check(_L.gs_convert_pods(self.sh, self.cov, to.sh, to.cov, _ptr(pods) if n else _ptr(out), n, _ptr(out)))
        return out[:n * to.size]

    def decompose(self, pods, to_sh):
        """gs_decompose_pods: packed records of this layout -> packed records of layout (to_sh, rotation +
        scale), on the host, with the per-record function the device kernel calls: the covariance of a covariance layout
        goes through cov3d_decompose; a rotation + scale source is convert().  Defined for every layout."""
        to = GaussianPod(to_sh, COV3D_ROT_SCALE)
        pods = np.ascontiguousarray(pods, dtype=np.uint8).reshape(-1)
        if pods.size % self.size:
            raise ValueError("%d bytes are no whole number of %d-byte records" % (pods.size, self.size))
        n = pods.size // self.size
        out = np.zeros(max(n * to.size, 1), dtype=np.uint8)
        _check(_L.gs_decompose_pods(self.sh, self.cov, to.sh, _ptr(pods) if n else _ptr(out), n, _ptr(out)))
        return out[:n * to.size]

    def __repr__(self):
        return self.name

    def __eq__(self, o):
        return isinstance(o, GaussianPod) and (self.sh, self.cov) == (o.sh, o.cov)

    def __hash__(self):
        return hash((self.sh, self.cov))


ALL_PODS = [GaussianPod(s, c) for s in range(4) for c in range(3)]
for _p in ALL_PODS:
    globals()[_p.name] = _p


class GaussianShDegree:
    """src/buffer/gaussian_transform.rs:17-52"""

    def __init__(self, v):
        self.v = int(v)

    @staticmethod
    def new(sh_deg):
        return GaussianShDegree(sh_deg) if 0 <= sh_deg <= 3 else None

    def get(self):
        return self.v


class GaussianMaxStdDev:
    """src/buffer/gaussian_transform.rs:55-98"""

    def __init__(self, u8):
        self.u8 = int(u8)

    @staticmethod
    def new(max_std_dev):
        out = C.c_uint8()
        if _L.gs_max_std_dev_encode(max_std_dev, C.byref(out)) != 0:
            return None
        return GaussianMaxStdDev(out.value)

    def get(self):
        return _L.gs_max_std_dev_decode(self.u8)

    def as_u8(self):
        return self.u8


def gaussian_transform_pod(size=1.0, display_mode=DISPLAY_SPLAT, sh_deg=3, no_sh0=False,
                           max_std_dev=3.0):
    """GaussianTransformPod::new — raises InvalidArgumentError where the Rust newtypes return None."""
    pod = GaussianTransformPod()
    _check(_L.gs_gaussian_transform_pod_new(size, display_mode, sh_deg, int(bool(no_sh0)),
                                            max_std_dev, C.byref(pod)))
    return pod


def model_transform_pod(pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0, 1.0), scale=(1.0, 1.0, 1.0)):
    """ModelTransformPod::new — src/buffer/model_transform.rs:68-77"""
    pod = ModelTransformPod()
    _L.gs_model_transform_pod_new(_ptr(np.asarray(pos, np.float32)), _ptr(np.asarray(rot, np.float32)),
                                  _ptr(np.asarray(scale, np.float32)), C.byref(pod))
    return pod


def camera_look_at(eye, target, up, vfov_radians, width, height, near=0.1, far=100.0,
                   background=(0.0, 0.0, 0.0)):
    cam = Camera()
    _L.gs_camera_look_at(_ptr(np.asarray(eye, np.float32)), _ptr(np.asarray(target, np.float32)),
                         _ptr(np.asarray(up, np.float32)), vfov_radians, width, height, near, far,
                         C.byref(cam))
    cam.background[:] = background
    return cam


# ------------------------------------------------------------------------------------------------
# PLY source format — src/source_format/ply.rs
# ------------------------------------------------------------------------------------------------

#: PlyGaussianPod — src/source_format/ply.rs:11-21
PLY_GAUSSIAN_DTYPE = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("color", "<f4", 3),
                               ("sh", "<f4", 45), ("alpha", "<f4"), ("scale", "<f4", 3), ("rot", "<f4", 4)])
PLY_PROPERTIES = [_L.gs_ply_property_name(i).decode() for i in range(62)]


def gaussian_from_ply(ply):
    """Gaussian::from_ply over an array of PlyGaussianPod"""
    p = np.ascontiguousarray(np.atleast_1d(ply), dtype=PLY_GAUSSIAN_DTYPE)
    out = np.zeros(len(p), dtype=GAUSSIAN_DTYPE)
    _L.gs_gaussian_from_ply(_ptr(p), len(p), _ptr(out))
    return out


def expf(x):
    """gs_expf: the exp of Gaussian::from_ply on host and device (csrc/gs_convert.h)"""
    return float(_L.gs_expf(float(x)))


def logf(x):
    """gs_logf: the ln of Gaussian::to_ply / to_spz on host and device (csrc/gs_convert.h)"""
    return float(_L.gs_logf(float(x)))


def cov3d_decompose(cov):
    """gs_cov3d_decompose: the six binary32 terms xx, yx, zx, yy, zy, zz of one covariance, or an (n, 6)
    array of them -> (rot xyzw, scale) as float32 arrays of shape (4,), (3,) or (n, 4), (n, 3).  The function the records
    of GaussianPod.decompose and GaussiansBuffer.decompose go through, on the host."""
    c = np.ascontiguousarray(cov, dtype=np.float32)
    if c.shape[-1:] != (6,) or c.ndim > 2:
        raise ValueError("a covariance has 6 terms; got an array of shape %r" % (c.shape,))
    rows = c.reshape(-1, 6)
    rot, scale = np.zeros((len(rows), 4), np.float32), np.zeros((len(rows), 3), np.float32)
    for i in range(len(rows)):
        _L.gs_cov3d_decompose(_ptr(rows[i]), _ptr(rot[i]), _ptr(scale[i]))
    return (rot[0], scale[0]) if c.ndim == 1 else (rot, scale)


def gaussian_to_ply(gaussians):
    """Gaussian::to_ply"""
    g = np.ascontiguousarray(np.atleast_1d(gaussians), dtype=GAUSSIAN_DTYPE)
    out = np.zeros(len(g), dtype=PLY_GAUSSIAN_DTYPE)
    _L.gs_gaussian_to_ply(_ptr(g), len(g), _ptr(out))
    return out


class PlyGaussians:
    """PlyGaussians — src/source_format/ply.rs:200-449 (a Vec<PlyGaussianPod> with I/O)."""

    def __init__(self, pods, inria=None):
        self.pods = np.ascontiguousarray(pods, dtype=PLY_GAUSSIAN_DTYPE)
        self.inria = inria

    def __len__(self):
        return len(self.pods)

    def is_empty(self):
        return len(self.pods) == 0

    @staticmethod
    def read_from(data):
        """ReadIterGaussian::read_from on a bytes-like object"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        n, inria = C.c_size_t(), C.c_int32()
        _check(_L.gs_ply_read(_ptr(buf), buf.size, None, 0, C.byref(n), C.byref(inria)))
        pods = np.zeros(n.value, dtype=PLY_GAUSSIAN_DTYPE)
        _check(_L.gs_ply_read(_ptr(buf), buf.size, _ptr(pods), n.value, C.byref(n), C.byref(inria)))
        return PlyGaussians(pods, bool(inria.value))

    @staticmethod
    def read_from_file(path):
        with open(path, "rb") as f:
            return PlyGaussians.read_from(f.read())

    @staticmethod
    def from_gaussians(gaussians):
        """FromIterator<Gaussian>"""
        return PlyGaussians(gaussian_to_ply(gaussians))

    def write_to(self):
        """WriteIterGaussian::write_to -> bytes"""
        n = C.c_size_t()
        _check(_L.gs_ply_write(_ptr(self.pods), len(self.pods), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        _check(_L.gs_ply_write(_ptr(self.pods), len(self.pods), _ptr(out), out.size, C.byref(n)))
        return out.tobytes()

    def write_to_file(self, path):
        with open(path, "wb") as f:
            f.write(self.write_to())

    def iter_gaussian(self):
        """IterGaussian: the Gaussians (Gaussian::from_ply of every pod)"""
        return gaussian_from_ply(self.pods)

    def __eq__(self, o):
        return isinstance(o, PlyGaussians) and self.pods.tobytes() == o.pods.tobytes()


# ------------------------------------------------------------------------------------------------
# SPZ source format — src/source_format/spz.rs
# ------------------------------------------------------------------------------------------------

def spz_options(version=3, sh_degree=3, fractional_bits=12, antialiased=False, sh_quantize_bits=(5, 4, 4)):
    """SpzGaussiansFromGaussianSliceOptions (defaults as the reference's)"""
    o = _capi.SpzOptions()
    _L.gs_spz_options_default(C.byref(o))
    o.version, o.sh_degree, o.fractional_bits = version, sh_degree, fractional_bits
    o.antialiased = int(bool(antialiased))
    o.sh_quantize_bits[:] = list(sh_quantize_bits)
    return o


def _sized_call(fn, *head):
    """two-call pattern of the C ABI: size query with out == NULL, then fill"""
    n = C.c_size_t()
    _check(fn(*head, None, 0, C.byref(n)))
    out = np.zeros(max(n.value, 1), dtype=np.uint8)
    _check(fn(*head, _ptr(out), n.value, C.byref(n)))
    return out[:n.value].tobytes()


_new_bytearray = C.pythonapi.PyByteArray_FromStringAndSize      # (NULL, n): n bytes, contents not initialised
_new_bytearray.restype = C.py_object
_new_bytearray.argtypes = [C.c_char_p, C.c_ssize_t]


def _bounded_call(fn, bound, *head):
    """One call with room for the largest result (a size query of the fast gzip member would encode twice).  Returns a
    bytearray cut to the result in place: copying half a gigabyte into a bytes object costs more than encoding it."""
    n = C.c_size_t()
    # uninitialised: bytearray(n) would write n zeroes, and at half a gigabyte touching the pages costs more than the call
    out = _new_bytearray(None, max(int(bound), 1))
    view = np.frombuffer(out, dtype=np.uint8)
    try:
        _check(fn(*head, _ptr(view), view.size, C.byref(n)))
    finally:
        del view                             # a bytearray with an exported buffer cannot be resized
    del out[n.value:]
    return out


def gzip_fast_bound(n):
    """gs_gzip_fast_bound: the largest member of n input bytes"""
    return _L.gs_gzip_fast_bound(int(n))


def gzip_fast(data):
    """gs_gzip_fast: `data` as a Huffman-only gzip member, encoded on the host — what Buffer.gzip_fast
    gives for the same bytes on the device.  Any inflater reads it; it is not the bytes of zlib's encoder.  Returns a
    bytearray (bytes-like: compare it, write it to a file, inflate it)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    return _bounded_call(_L.gs_gzip_fast, gzip_fast_bound(buf.size), _ptr(buf) if buf.size else None, buf.size)


class SpzGaussians:
    """SpzGaussians — spz.rs:514-959.  Holds the decompressed payload (header + columns) exactly as
    read or encoded, so write_to reproduces the same columns; `gaussians` is Gaussian::from_spz of
    every point (what iter_gaussian yields)."""

    def __init__(self, payload):
        self.payload = bytes(payload)
        buf = np.frombuffer(self.payload, dtype=np.uint8)
        hdr, n = _capi.SpzHeader(), C.c_size_t()
        _check(_L.gs_spz_decode_decompressed(_ptr(buf), buf.size, C.byref(hdr), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=GAUSSIAN_DTYPE)
        _check(_L.gs_spz_decode_decompressed(_ptr(buf), buf.size, C.byref(hdr), _ptr(out), n.value, C.byref(n)))
        self.header, self.gaussians = hdr, out

    def __len__(self):
        return len(self.gaussians)

    def is_empty(self):
        return len(self.gaussians) == 0

    def __eq__(self, o):
        return isinstance(o, SpzGaussians) and self.payload == o.payload

    # ---- reading
    @staticmethod
    def read_from(data):
        """ReadIterGaussian::read_from (gzip'd .spz bytes)"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        return SpzGaussians(_sized_call(_L.gs_spz_decompress, _ptr(buf), buf.size))

    @staticmethod
    def read_decompressed(data):
        return SpzGaussians(data)

    @staticmethod
    def read_from_file(path):
        with open(path, "rb") as f:
            return SpzGaussians.read_from(f.read())

    # ---- from Gaussians
    @staticmethod
    def from_gaussians_with_options(gaussians, options=None):
        """from_gaussians_with_options (spz.rs:806-835); from_gaussians / FromIterator use the defaults"""
        return SpzGaussians(SpzGaussians.write_gaussians_decompressed(gaussians, options))

    from_gaussians = from_gaussians_with_options

    def iter_gaussian(self):
        return self.gaussians

    # ---- writing
    def write_decompressed(self):
        return self.payload

    def write_to(self):
        """WriteIterGaussian::write_to -> gzip'd bytes"""
        buf = np.frombuffer(self.payload, dtype=np.uint8)
        return _sized_call(_L.gs_spz_compress, _ptr(buf), buf.size)

    def write_to_file(self, path):
        with open(path, "wb") as f:
            f.write(self.write_to())

    # ---- one-shot helpers over the C ABI's fused entry points
    @staticmethod
    def _encode(fn, gaussians, options):
        g = np.ascontiguousarray(np.atleast_1d(gaussians), dtype=GAUSSIAN_DTYPE)
        options = options or spz_options()
        return _sized_call(fn, _ptr(g), len(g), C.byref(options))

    @staticmethod
    def write_gaussians(gaussians, options=None):
        """from_gaussians_with_options + write_to -> gzip'd bytes (gs_spz_encode)"""
        return SpzGaussians._encode(_L.gs_spz_encode, gaussians, options)

    @staticmethod
    def write_gaussians_decompressed(gaussians, options=None):
        return SpzGaussians._encode(_L.gs_spz_encode_decompressed, gaussians, options)

    @staticmethod
    def decode(data):
        """gs_spz_decode: gzip'd bytes -> (header, Gaussians) in one call"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        hdr, n = _capi.SpzHeader(), C.c_size_t()
        _check(_L.gs_spz_decode(_ptr(buf), buf.size, C.byref(hdr), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=GAUSSIAN_DTYPE)
        _check(_L.gs_spz_decode(_ptr(buf), buf.size, C.byref(hdr), _ptr(out), n.value, C.byref(n)))
        return hdr, out


class GaussiansSource:
    """GaussiansSource — src/gaussian.rs:394-416"""
    Internal, Ply, Spz = "Internal", "Ply", "Spz"


class Gaussians:
    """Gaussians — the unified representation (src/gaussian.rs:412-548): Internal holds an array of
    Gaussian, Ply a PlyGaussians, Spz a SpzGaussians."""

    def __init__(self, inner):
        if isinstance(inner, Gaussians):
            inner = inner.inner
        if not isinstance(inner, (PlyGaussians, SpzGaussians)):
            inner = np.ascontiguousarray(np.atleast_1d(inner), dtype=GAUSSIAN_DTYPE)   # From<Vec<Gaussian>>
        self.inner = inner

    @staticmethod
    def from_gaussians_iter(gaussians, source):
        g = np.ascontiguousarray(np.atleast_1d(gaussians), dtype=GAUSSIAN_DTYPE)
        if source == GaussiansSource.Internal:
            return Gaussians(g)
        if source == GaussiansSource.Ply:
            return Gaussians(PlyGaussians.from_gaussians(g))
        if source == GaussiansSource.Spz:
            return Gaussians(SpzGaussians.from_gaussians(g))
        raise ValueError("unknown GaussiansSource %r" % (source,))

    def source(self):
        if isinstance(self.inner, PlyGaussians):
            return GaussiansSource.Ply
        if isinstance(self.inner, SpzGaussians):
            return GaussiansSource.Spz
        return GaussiansSource.Internal

    def __len__(self):
        return len(self.inner)

    def is_empty(self):
        return len(self.inner) == 0

    @staticmethod
    def read_from(data, source):
        if source == GaussiansSource.Internal:
            raise ValueError("cannot read Internal Gaussians from buffer")      # gaussian.rs:480-483
        cls = PlyGaussians if source == GaussiansSource.Ply else SpzGaussians
        return Gaussians(cls.read_from(data))

    @staticmethod
    def read_from_file(path, source):
        if source == GaussiansSource.Internal:
            raise ValueError("cannot read Internal Gaussians from file")        # gaussian.rs:461-464
        cls = PlyGaussians if source == GaussiansSource.Ply else SpzGaussians
        return Gaussians(cls.read_from_file(path))

    def write_to(self):
        if self.source() == GaussiansSource.Internal:
            raise ValueError("cannot write Internal Gaussians to buffer")       # gaussian.rs:510-513
        return self.inner.write_to()

    def write_to_file(self, path):
        if self.source() == GaussiansSource.Internal:
            raise ValueError("cannot write Internal Gaussians to file")         # gaussian.rs:498-501
        self.inner.write_to_file(path)

    def iter_gaussian(self):
        """IterGaussian — the Gaussians in the internal format, whatever the source"""
        return self.inner if self.source() == GaussiansSource.Internal else self.inner.iter_gaussian()

    def __eq__(self, o):
        if not isinstance(o, Gaussians) or self.source() != o.source():
            return False
        if self.source() == GaussiansSource.Internal:
            return self.inner.tobytes() == o.inner.tobytes()
        return self.inner == o.inner


# ------------------------------------------------------------------------------------------------
# device / stream / buffers
# ------------------------------------------------------------------------------------------------

def hip_versions():
    """(compiled, runtime, driver): HIP_VERSION of the headers libgs3d_hip.so was built with and the
    versions of the runtime / driver it runs on (gs_hip_versions; wgpu AdapterInfo::driver_info)."""
    a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _L.gs_hip_versions(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


class Device:
    """wgpu::Device + wgpu::Queue."""

    def __init__(self, ordinal=0):
        h = C.c_void_p()
        _check(_L.gs_device_create(ordinal, C.byref(h)))
        self._h = h
        self.ordinal = ordinal

    def limits(self):
        lim = Limits()
        _check(_L.gs_device_limits(self._h, C.byref(lim)))
        return lim

    def synchronize(self):
        _check(_L.gs_device_synchronize(self._h))

    def fast_rank(self):
        """True while this device's radix sorts rank with returning LDS atomics (gs_device_fast_rank)"""
        return bool(_L.gs_device_fast_rank(self._h))

    def create_stream(self, priority=None):
        """priority: see gs_stream_create_with_priority — streams meant to overlap on the device (frames in flight)
        need different priorities to be sure of different hardware queues"""
        return Stream(self, priority=priority)

    def stream_priority_range(self):
        """(least, greatest) of hipDeviceGetStreamPriorityRange; numerically lower = higher priority"""
        lo, hi = C.c_int32(0), C.c_int32(0)
        _check(_L.gs_device_stream_priority_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def wrap_stream(self, native_handle):
        return Stream(self, native=native_handle)

    def close(self):
        if self._h:
            _L.gs_device_destroy(self._h)
            self._h = None


class Stream:
    """CommandEncoder + queue.submit: an ordered HIP stream."""

    def __init__(self, device, native=None, priority=None):
        h = C.c_void_p()
        if native is None and priority is not None:
            _check(_L.gs_stream_create_with_priority(device._h, int(priority), C.byref(h)))
        elif native is None:
            _check(_L.gs_stream_create(device._h, C.byref(h)))
        else:
            _check(_L.gs_stream_wrap(device._h, C.c_void_p(native), C.byref(h)))
        self._h = h
        self.device = device

    def synchronize(self):
        _check(_L.gs_stream_synchronize(self._h))

    def native(self):
        return _L.gs_stream_native(self._h)

    def close(self):
        if self._h:
            _L.gs_stream_destroy(self._h)
            self._h = None


class Buffer:
    """wgpu::Buffer with the BufferWrapper download contract (src/buffer/mod.rs:17-102)."""

    def __init__(self, device, size=None, data=None, _handle=None):
        self.device = device
        if _handle is not None:
            self._h = _handle
            return
        h = C.c_void_p()
        if data is not None:
            data = np.ascontiguousarray(data)
            size = data.nbytes
        _check(_L.gs_buffer_create(device._h, size, _ptr(data) if data is not None else None,
                                   C.byref(h)))
        self._h = h

    @staticmethod
    def from_raw(device, device_ptr, size):
        h = C.c_void_p()
        _check(_L.gs_buffer_from_raw(device._h, C.c_void_p(device_ptr), size, C.byref(h)))
        return Buffer(device, _handle=h)

    def clone(self):
        return Buffer(self.device, _handle=C.c_void_p(_L.gs_buffer_retain(self._h)))

    def size(self):
        return _L.gs_buffer_size(self._h)

    def device_ptr(self):
        return _L.gs_buffer_device_ptr(self._h)

    def write(self, stream, offset, data):
        data = np.ascontiguousarray(data)
        _check(_L.gs_buffer_write(self._h, stream._h, offset, _ptr(data), data.nbytes))

    def download(self, stream, dtype=np.uint8):
        """BufferWrapper::download::<T> — blocking."""
        out = np.zeros(self.size(), dtype=np.uint8)
        _check(_L.gs_buffer_download(self._h, stream._h, _ptr(out), out.nbytes))
        return out.view(dtype)

    def gzip_fast(self, stream, offset=0, length=None):
        """gs_buffer_gzip_fast: the bytes [offset, offset + length) of the buffer (None: to its end) as a
        Huffman-only gzip member, deflated on the device; only the member crosses the link.  Byte-equal to
        gzip_fast(those bytes), and a bytearray like it.  Blocking."""
        if stream is not None and not isinstance(stream, Stream):
            raise TypeError("stream must be a Stream or None, not %s" % type(stream).__name__)
        offset = int(offset)
        length = self.size() - offset if length is None else int(length)
        if offset < 0 or length < 0:
            raise ValueError("offset and length must not be negative")
        # a range past the buffer is the library's to refuse: no room is made for it
        return _bounded_call(_L.gs_buffer_gzip_fast, gzip_fast_bound(min(length, self.size())), self._h, stream._h if stream is not None else None,
                             offset, length)

    def prepare_download(self, stream):
        """BufferWrapper::prepare_download: enqueue the copy into a staging buffer; returns a Download"""
        h = C.c_void_p()
        _check(_L.gs_buffer_prepare_download(self._h, stream._h if stream else None, C.byref(h)))
        return Download(h)

    def release(self):
        if self._h:
            _L.gs_buffer_release(self._h)
            self._h = None


class Download:
    """A pending device-to-host copy (gs_download): map() = BufferWrapper::map_download"""

    def __init__(self, handle):
        self._h = handle

    def ready(self):
        return bool(_L.gs_download_ready(self._h))

    def map(self, dtype=np.uint8):
        """blocks until the copy has landed; returns a numpy COPY of the staged bytes"""
        data, n = C.c_void_p(), C.c_size_t()
        _check(_L.gs_download_map(self._h, C.byref(data), C.byref(n)))
        raw = (C.c_uint8 * n.value).from_address(data.value) if n.value else b""
        return np.frombuffer(bytes(raw), dtype=np.uint8).view(dtype).copy()

    def release(self):
        if self._h:
            _L.gs_download_release(self._h)
            self._h = None


def pack_device(device, stream, pod, gaussians_buffer, count, pods_buffer):
    """gs_pack_device: Gaussians (struct Gaussian records in `gaussians_buffer`) -> PODs in `pods_buffer`"""
    _check(_L.gs_pack_device(device._h, stream._h if stream else None, pod.sh, pod.cov,
                             C.c_void_p(gaussians_buffer.device_ptr()), count, C.c_void_p(pods_buffer.device_ptr())))


NEIGHBOR_COUNT_MAX = 0xFFFFFFFF      # UINT32_MAX: no cap / no upper limit
COMPONENT_NONE = 0xFFFFFFFF          # GS_COMPONENT_NONE: the label of a Gaussian that is no point
# gs_components_info: what GaussiansBuffer.components writes into its info Buffer
COMPONENTS_INFO_DTYPE = np.dtype([("points", "<u4"), ("components", "<u4"), ("largest", "<u4"), ("largest_label", "<u4")])


def _neighbor_args(radius, among, model_transform):
    """(radius, among handle or None, transform reference or None) of the neighbour calls, checked before any library
    call: a finite radius >= 0 whose binary32 square is finite, a Selection or None, a ModelTransformPod or None."""
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise TypeError("radius must be a number, not %s" % type(radius).__name__)
    r = np.float32(radius)
    with np.errstate(over="ignore"):
        if not (np.isfinite(r) and r >= 0 and np.isfinite(r * r)):
            raise ValueError("radius must be finite and >= 0, with a finite square in binary32, not %r" % (radius,))
    if among is not None and not isinstance(among, Selection):
        raise TypeError("among must be a Selection or None, not %s" % type(among).__name__)
    if model_transform is not None and not isinstance(model_transform, ModelTransformPod):
        raise TypeError("model_transform must be a ModelTransformPod or None, not %s" % type(model_transform).__name__)
    return (float(r), among._h if among is not None else None,
            C.byref(model_transform) if model_transform is not None else None)


KNN_NONE = 0xFFFFFFFF                # GS_KNN_NONE: the index of a padding entry of a k-NN row
KNN_MAX_K = 16                       # GS_KNN_MAX_K
KNN_KTH_DIST2, KNN_MEAN_DIST = 0, 1  # GS_KNN_*: the statistic select_knn / knn_summary take of a row
_KNN_KINDS = {"kth_dist2": KNN_KTH_DIST2, "mean_dist": KNN_MEAN_DIST}


def _knn_k(k):
    """k of the k-NN calls, checked before any library call: an integer in 1..KNN_MAX_K"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError("k must be an integer, not %s" % type(k).__name__)
    if not 1 <= int(k) <= KNN_MAX_K:
        raise ValueError("k must be between 1 and %d, not %d" % (KNN_MAX_K, k))
    return int(k)


def knn_kind(kind):
    """GS_KNN_* from its number or name ('kth_dist2', 'mean_dist'); ValueError for anything else."""
    if isinstance(kind, str) and kind.lower() in _KNN_KINDS:
        return _KNN_KINDS[kind.lower()]
    if isinstance(kind, (int, np.integer)) and not isinstance(kind, bool) and int(kind) in (KNN_KTH_DIST2, KNN_MEAN_DIST):
        return int(kind)
    raise ValueError("unknown k-NN statistic %r (one of %s)" % (kind, ", ".join(_KNN_KINDS)))


@dataclasses.dataclass
class KnnSummary:
    """gs_knn_summary_result: the rows of a distance plane that are a point's, those that are complete, and over the
    complete rows' statistic v its bit-defined min and max (+inf / -inf without one) and the binary64 sums of v and v v."""
    points: int
    complete: int
    min: np.float32
    max: np.float32
    sum: float
    sum_sq: float

    @property
    def mean(self):
        return self.sum / self.complete if self.complete else float("nan")

    @property
    def std(self):
        """the population standard deviation, in binary64"""
        if not self.complete:
            return float("nan")
        return float(np.sqrt(max(self.sum_sq / self.complete - self.mean * self.mean, 0.0)))


def knn_summary(stream, dist2_plane, n, k, kind=KNN_KTH_DIST2):
    """gs_knn_summary: a KnnSummary of the statistic `kind` (KNN_KTH_DIST2, KNN_MEAN_DIST or their
    names) over the n rows of k values of `dist2_plane`, a Buffer GaussiansBuffer.knn filled.  Blocking."""
    if stream is not None and not isinstance(stream, Stream):
        raise TypeError("stream must be a Stream or None, not %s" % type(stream).__name__)
    if not isinstance(dist2_plane, Buffer):
        raise TypeError("dist2_plane must be a Buffer, not %s" % type(dist2_plane).__name__)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise TypeError("n must be an integer, not %s" % type(n).__name__)
    if int(n) < 0:
        raise ValueError("n must be >= 0, not %d" % n)
    k, kind = _knn_k(k), knn_kind(kind)
    out = _capi.KnnSummaryRecord()
    _check(_L.gs_knn_summary(stream._h if stream is not None else None, dist2_plane._h, int(n), k, kind, C.byref(out)))
    return KnnSummary(points=int(out.points), complete=int(out.complete), min=np.float32(out.min), max=np.float32(out.max),
                      sum=float(out.sum), sum_sq=float(out.sum_sq))


@dataclasses.dataclass
class PairSums:
    """gs_pair_sums: the number of pairs (p of the query side, q of the target side) and the binary64 sums
    of p, q, p_a q_b (3 x 3, row a), |p|^2, |q|^2 and |p - q|^2 over them."""
    pairs: int
    sp: np.ndarray
    sq: np.ndarray
    spq: np.ndarray
    spp: float
    sqq: float
    sdd: float

    @property
    def rms(self):
        """sqrt(sdd / pairs): the RMS distance of the pairs; NaN without one"""
        return float(np.sqrt(self.sdd / self.pairs)) if self.pairs else float("nan")

    def record(self):
        """the 152 bytes of the C record"""
        r = _capi.PairSumsRecord()
        r.pairs = int(self.pairs)
        r.sp[:] = [float(v) for v in np.asarray(self.sp, np.float64).reshape(3)]
        r.sq[:] = [float(v) for v in np.asarray(self.sq, np.float64).reshape(3)]
        r.spq[:] = [float(v) for v in np.asarray(self.spq, np.float64).reshape(9)]
        r.spp, r.sqq, r.sdd = float(self.spp), float(self.sqq), float(self.sdd)
        return r

    @staticmethod
    def from_record(r):
        return PairSums(pairs=int(r.pairs), sp=np.array(r.sp[:], np.float64), sq=np.array(r.sq[:], np.float64),
                        spq=np.array(r.spq[:], np.float64).reshape(3, 3), spp=float(r.spp), sqq=float(r.sqq), sdd=float(r.sdd))


def rigid_fit(sums, scale=False):
    """gs_rigid_fit: (delta, rms).  delta: the ModelTransformPod of the rotation, translation and — with
    scale=True — uniform scale that brings the p of the pairs of `sums` (a PairSums) onto their q in the least-squares
    sense, Horn's closed form in binary64 on the host; it acts in world space AFTER the query side's transform
    (compose_model_transform).  rms: sqrt(sdd / pairs) of the pairs as they came in.  InvalidArgumentError for fewer than
    3 pairs, a sum that is not finite, or pairs that determine no rotation."""
    if not isinstance(sums, PairSums):
        raise TypeError("sums must be a PairSums, not %s" % type(sums).__name__)
    if not isinstance(scale, bool):
        raise TypeError("scale must be a bool, not %s" % type(scale).__name__)
    rec, delta, rms = sums.record(), ModelTransformPod(), C.c_double()
    _check(_L.gs_rigid_fit(C.byref(rec), 1 if scale else 0, C.byref(delta), C.byref(rms)))
    return delta, rms.value


def compose_model_transform(delta, m):
    """gs_model_transform_compose: the ModelTransformPod of delta o m for a `delta` of uniform scale:
    rot = r_d r, scale = s_d scale, pos = s_d R_d pos + t_d."""
    for name, v in (("delta", delta), ("m", m)):
        if not isinstance(v, ModelTransformPod):
            raise TypeError("%s must be a ModelTransformPod, not %s" % (name, type(v).__name__))
    out = ModelTransformPod()
    _L.gs_model_transform_compose(C.byref(delta), C.byref(m), C.byref(out))
    return out


@dataclasses.dataclass
class Chamfer:
    """What GaussiansBuffer.chamfer_to returns: the KnnSummary (k = 1, KNN_MEAN_DIST) of each direction.  mean_*: the mean
    distance to the nearest Gaussian of the other buffer over those that have one within the radius (NaN without any);
    incomplete_*: the Gaussians with a finite position that have none."""
    to_target: KnnSummary
    from_target: KnnSummary

    @property
    def mean_to(self):
        return self.to_target.mean

    @property
    def mean_from(self):
        return self.from_target.mean

    @property
    def incomplete_to(self):
        return self.to_target.points - self.to_target.complete

    @property
    def incomplete_from(self):
        return self.from_target.points - self.from_target.complete

    @property
    def distance(self):
        """the symmetric Chamfer distance: mean_to + mean_from"""
        return self.mean_to + self.mean_from


@dataclasses.dataclass
class AlignReport:
    """What GaussiansBuffer.align_to did: one (pairs, rms) entry per iteration, measured BEFORE that iteration's fit, and why
    it stopped: 'converged' (the RMS fell by less than rms_tol of itself), 'pairs' (fewer than 3) or 'iterations'."""
    iterations: list
    stopped: str


class GaussiansBuffer:
    """GaussiansBuffer<G> — src/buffer/gaussian.rs:17-229."""

    def __init__(self, device, pod, _handle):
        self.device, self.pod, self._h = device, pod, _handle

    @staticmethod
    def new(device, pod, gaussians):
        g = np.ascontiguousarray(np.atleast_1d(gaussians), dtype=GAUSSIAN_DTYPE)
        h = C.c_void_p()
        _check(_L.gs_gaussians_buffer_create_from_gaussians(device._h, pod.sh, pod.cov, _ptr(g),
                                                            len(g), C.byref(h)))
        return GaussiansBuffer(device, pod, h)

    @staticmethod
    def new_from_ply(device, pod, ply):
        """PlyGaussians (or an array of PlyGaussianPod) -> buffer: the vertex records are uploaded as
        they are and ONE device kernel does Gaussian::from_ply + G::from_gaussian
        (gs_gaussians_buffer_create_from_ply) — bit-equal to new(device, pod, gaussian_from_ply(ply))."""
        p = np.ascontiguousarray(np.atleast_1d(getattr(ply, "pods", ply)), dtype=PLY_GAUSSIAN_DTYPE)
        h = C.c_void_p()
        _check(_L.gs_gaussians_buffer_create_from_ply(device._h, pod.sh, pod.cov, _ptr(p), len(p), C.byref(h)))
        return GaussiansBuffer(device, pod, h)

    @staticmethod
    def new_from_spz(device, pod, data, decompressed=False):
        """SPZ file bytes (gzip'd, or the decompressed payload) -> buffer: inflate on the host, then ONE
        device kernel does Gaussian::from_spz + G::from_gaussian (gs_gaussians_buffer_create_from_spz) —
        bit-equal to new(device, pod, SpzGaussians.read_from(data).iter_gaussian())."""
        raw = np.frombuffer(bytes(data), dtype=np.uint8)
        h, hdr = C.c_void_p(), _capi.SpzHeader()
        fn = _L.gs_gaussians_buffer_create_from_spz_decompressed if decompressed else _L.gs_gaussians_buffer_create_from_spz
        _check(fn(device._h, pod.sh, pod.cov, _ptr(raw), raw.size, C.byref(hdr), C.byref(h)))
        b = GaussiansBuffer(device, pod, h)
        b.spz_header = hdr
        return b

    @staticmethod
    def new_with_pods(device, pod, pods):
        pods = np.ascontiguousarray(pods, dtype=np.uint8)
        assert pods.nbytes % pod.size == 0
        h = C.c_void_p()
        _check(_L.gs_gaussians_buffer_create(device._h, pod.sh, pod.cov, _ptr(pods),
                                             pods.nbytes // pod.size, C.byref(h)))
        return GaussiansBuffer(device, pod, h)

    @staticmethod
    def new_empty(device, pod, length):
        h = C.c_void_p()
        _check(_L.gs_gaussians_buffer_create(device._h, pod.sh, pod.cov, None, length, C.byref(h)))
        return GaussiansBuffer(device, pod, h)

    @staticmethod
    def try_from(buffer, pod):
        """TryFrom<wgpu::Buffer> — raises GaussiansBufferTryFromBufferError."""
        h = C.c_void_p()
        _check(_L.gs_gaussians_buffer_from_buffer(buffer._h, pod.sh, pod.cov, C.byref(h)))
        return GaussiansBuffer(buffer.device, pod, h)

    def len(self):
        return _L.gs_gaussians_buffer_len(self._h)

    __len__ = len

    def is_empty(self):
        return self.len() == 0

    def buffer(self):
        """BufferWrapper::buffer() — a new handle to the same device allocation."""
        return Buffer(self.device, _handle=C.c_void_p(
            _L.gs_buffer_retain(_L.gs_gaussians_buffer_buffer(self._h))))

    def update(self, stream, gaussians):
        g = np.ascontiguousarray(np.atleast_1d(gaussians), dtype=GAUSSIAN_DTYPE)
        _check(_L.gs_gaussians_buffer_update_gaussians(self._h, stream._h, _ptr(g), len(g)))

    def update_with_pod(self, stream, pods):
        pods = np.ascontiguousarray(pods, dtype=np.uint8)
        _check(_L.gs_gaussians_buffer_update(self._h, stream._h, _ptr(pods),
                                             pods.nbytes // self.pod.size))

    def update_range(self, stream, start, gaussians):
        g = np.ascontiguousarray(np.atleast_1d(gaussians), dtype=GAUSSIAN_DTYPE)
        _check(_L.gs_gaussians_buffer_update_range_gaussians(self._h, stream._h, start, _ptr(g), len(g)))

    def update_range_from_ply(self, stream, start, ply):
        p = np.ascontiguousarray(np.atleast_1d(getattr(ply, "pods", ply)), dtype=PLY_GAUSSIAN_DTYPE)
        _check(_L.gs_gaussians_buffer_update_range_ply(self._h, stream._h, start, _ptr(p), len(p)))

    def update_range_with_pod(self, stream, start, pods):
        pods = np.ascontiguousarray(pods, dtype=np.uint8)
        _check(_L.gs_gaussians_buffer_update_range(self._h, stream._h, start, _ptr(pods),
                                                   pods.nbytes // self.pod.size))

    def download(self, stream):
        out = np.zeros(self.len() * self.pod.size, dtype=np.uint8)
        _check(_L.gs_gaussians_buffer_download(self._h, stream._h, _ptr(out), self.len()))
        return out

    def download_gaussians(self, stream):
        out = np.zeros(self.len(), dtype=GAUSSIAN_DTYPE)
        _check(_L.gs_gaussians_buffer_download_gaussians(self._h, stream._h, _ptr(out), self.len()))
        return out

    def mark_dirty(self):
        _L.gs_gaussians_buffer_mark_dirty(self._h)

    def set_spatial_order(self, enabled):
        """mirror slots in spatial (Morton) order (default) or in index order — DESIGN.md §3.4a"""
        _check(_L.gs_gaussians_buffer_set_spatial_order(self._h, int(bool(enabled))))

    def spatial_order(self):
        return bool(_L.gs_gaussians_buffer_spatial_order(self._h))

    def download_order(self, stream=None):
        """order[slot] = Gaussian index of the renderer's mirror (the identity in index order)"""
        out = np.zeros(self.len(), dtype=np.uint32)
        _check(_L.gs_gaussians_buffer_download_order(self._h, stream._h if stream is not None else None,
                                                      _ptr(out), self.len()))
        return out

    def edit(self, stream, selection, edit):
        """gs_gaussians_buffer_edit: applies `edit` (see edit()) to the Gaussians of `selection` (None:
        all) in place on the device.  Only enqueues on the stream; the next frame of any renderer sees the result."""
        if selection is not None and not isinstance(selection, Selection):
            raise TypeError("selection must be a Selection or None, not %s" % type(selection).__name__)
        if not isinstance(edit, Edit):
            raise TypeError("edit must be an Edit (see edit()), not %s" % type(edit).__name__)
        _check(_L.gs_gaussians_buffer_edit(self._h, stream._h if stream is not None else None,
                                           selection._h if selection is not None else None, C.byref(edit)))

    def extract(self, stream, selection, invert=False):
        """gs_gaussians_buffer_create_from_selection: a new GaussiansBuffer of the same layout with the records of
        `selection` (invert: of its complement) in caller order, bytes unchanged.  Blocking.  `extract(sel, invert=True)`
        deletes the selection, the pair (extract(sel), extract(sel, invert=True)) splits the buffer."""
        if selection is not None and not isinstance(selection, Selection):
            raise TypeError("selection must be a Selection or None, not %s" % type(selection).__name__)
        h, count = C.c_void_p(), C.c_uint64()
        _check(_L.gs_gaussians_buffer_create_from_selection(self._h, stream._h if stream is not None else None,
                                                            selection._h if selection is not None else None,
                                                            int(bool(invert)), C.byref(h), C.byref(count)))
        out = GaussiansBuffer(self.device, self.pod, h)
        assert out.len() == count.value
        return out

    def convert(self, stream, pod, selection=None, invert=False):
        """gs_gaussians_buffer_create_converted: a new GaussiansBuffer of layout `pod` with the converted
        records of `selection` (None: all; invert: of its complement) in caller order — extract() and the conversion in one
        pass on the device.  Blocking.  Raises LossyConfigError where pod.convertible_to is False."""
        if not isinstance(pod, GaussianPod):
            raise TypeError("pod must be a GaussianPod, not %s" % type(pod).__name__)
        if selection is not None and not isinstance(selection, Selection):
            raise TypeError("selection must be a Selection or None, not %s" % type(selection).__name__)
        h, count = C.c_void_p(), C.c_uint64()
        _check(_L.gs_gaussians_buffer_create_converted(self._h, stream._h if stream is not None else None,
                                                       selection._h if selection is not None else None,
                                                       int(bool(invert)), pod.sh, pod.cov, C.byref(h), C.byref(count)))
        out = GaussiansBuffer(self.device, pod, h)
        assert out.len() == count.value
        return out

    def decompose(self, stream, sh=None, selection=None, invert=False):
        """gs_gaussians_buffer_create_decomposed: a new GaussiansBuffer of layout (sh, rotation + scale)
        — sh=None: this buffer's SH config — with the records of `selection` (None: all; invert: of its complement) in
        caller order, the covariance of each decomposed into a unit quaternion and three scales on the device: the way from
        a covariance layout to export_ply / export_spz / write and into a rotation + scale scene.  Blocking.  Byte-equal to
        pod.decompose(pods, sh) on the host; for a rotation + scale source it is convert()."""
        pod = GaussianPod(self.pod.sh if sh is None else sh, COV3D_ROT_SCALE)
        if selection is not None and not isinstance(selection, Selection):
            raise TypeError("selection must be a Selection or None, not %s" % type(selection).__name__)
        h, count = C.c_void_p(), C.c_uint64()
        _check(_L.gs_gaussians_buffer_create_decomposed(self._h, stream._h if stream is not None else None,
                                                        selection._h if selection is not None else None,
                                                        int(bool(invert)), pod.sh, C.byref(h), C.byref(count)))
        out = GaussiansBuffer(self.device, pod, h)
        assert out.len() == count.value
        return out

    def _export_decomposed(self, stream, selection, invert, export):
        """decompose=True of the exports on a covariance layout: export(tmp) for a temporary rotation + scale buffer that
        holds the decomposed selection and is destroyed again"""
        tmp = self.decompose(stream, None, selection, invert)
        try:
            return export(tmp)
        finally:
            tmp.destroy()

    def _export_args(self, stream, selection):
        if selection is not None and not isinstance(selection, Selection):
            raise TypeError("selection must be a Selection or None, not %s" % type(selection).__name__)
        return self._h, stream._h if stream is not None else None, selection._h if selection is not None else None

    def export_ply(self, stream, selection=None, invert=False, decompose=False):
        """gs_gaussians_buffer_export_ply: the records of `selection` (None: all; invert: of its
        complement) as PlyGaussians in caller order — extract(), download_gaussians() and gaussian_to_ply() in one kernel on
        the device, byte-equal to them.  Blocking.  decompose=True exports a covariance layout through decompose() (DESIGN.md
        §3.12a) instead of raising LossyConfigError; an SH-less layout raises it either way."""
        if decompose and self.pod.cov != COV3D_ROT_SCALE:
            return self._export_decomposed(stream, selection, invert, lambda b: b.export_ply(stream))
        head = self._export_args(stream, selection) + (int(bool(invert)),)
        count = C.c_uint64()
        _check(_L.gs_gaussians_buffer_export_ply(*head, None, 0, C.byref(count)))
        pods = np.zeros(count.value, dtype=PLY_GAUSSIAN_DTYPE)
        if count.value:
            _check(_L.gs_gaussians_buffer_export_ply(*head, _ptr(pods), len(pods), C.byref(count)))
        return PlyGaussians(pods[:count.value], True)

    def export_spz(self, stream, selection=None, invert=False, options=None, decompose=False):
        """gs_gaussians_buffer_export_spz_decompressed: the records of `selection` as SpzGaussians (None:
        spz_options()), the columns encoded on the device — byte-equal to
        SpzGaussians.from_gaussians_with_options(extract().download_gaussians(), options).  Blocking.  decompose: as
        export_ply's."""
        if decompose and self.pod.cov != COV3D_ROT_SCALE:
            return self._export_decomposed(stream, selection, invert, lambda b: b.export_spz(stream, options=options))
        if options is not None and not isinstance(options, _capi.SpzOptions):
            raise TypeError("options must be spz_options(...) or None, not %s" % type(options).__name__)
        head = self._export_args(stream, selection) + (int(bool(invert)), C.byref(options) if options is not None else None)
        return SpzGaussians(_sized_call(_L.gs_gaussians_buffer_export_spz_decompressed, *head))

    def export_spz_file(self, stream, selection=None, invert=False, options=None, fast=True, decompose=False):
        """The .spz file image of the records of `selection` as bytes.  fast=True: gs_gaussians_buffer_export_spz_fast
         — the payload stays on the device and is deflated there, Huffman only; fast=False:
        gs_gaussians_buffer_export_spz, zlib on one host thread.  Both inflate to export_spz(...).payload.  Blocking.  The fast
        image comes as a bytearray, zlib's as bytes.  decompose: as export_ply's."""
        if decompose and self.pod.cov != COV3D_ROT_SCALE:
            return self._export_decomposed(stream, selection, invert, lambda b: b.export_spz_file(stream, options=options, fast=fast))
        if options is not None and not isinstance(options, _capi.SpzOptions):
            raise TypeError("options must be spz_options(...) or None, not %s" % type(options).__name__)
        args = self._export_args(stream, selection) + (int(bool(invert)),)
        head = args + (C.byref(options) if options is not None else None,)
        if not fast:
            return _sized_call(_L.gs_gaussians_buffer_export_spz, *head)
        # the payload's size comes from the scan alone; the member is bounded by it
        n = C.c_size_t()
        _check(_L.gs_gaussians_buffer_export_spz_decompressed(*head, None, 0, C.byref(n)))
        return _bounded_call(_L.gs_gaussians_buffer_export_spz_fast, gzip_fast_bound(n.value), *head)

    def write(self, stream, source, selection=None, invert=False, fast=False, decompose=False):
        """gs_gaussians_buffer_write: the complete file image of the records of `selection` as bytes —
        GaussiansSource.Ply: header + vertices; GaussiansSource.Spz: the gzip member, default options.  Blocking.
        fast=True makes the SPZ member export_spz_file's (deflated on the device, not zlib's bytes); a PLY
        image has nothing to compress and is the same either way.  decompose: as export_ply's."""
        if decompose and self.pod.cov != COV3D_ROT_SCALE:
            return self._export_decomposed(stream, selection, invert, lambda b: b.write(stream, source, fast=fast))
        if source == GaussiansSource.Internal:
            raise ValueError("cannot write Internal Gaussians to buffer")
        if source not in (GaussiansSource.Ply, GaussiansSource.Spz):
            raise TypeError("source must be GaussiansSource.Ply or GaussiansSource.Spz, not %r" % (source,))
        if fast and source == GaussiansSource.Spz:
            return self.export_spz_file(stream, selection, invert, None, fast=True)
        args = self._export_args(stream, selection) + (int(bool(invert)),)
        head = args + (1 if source == GaussiansSource.Ply else 2,)
        if source == GaussiansSource.Spz:
            # A size query of the gzip member has to build it: ask for the size of the payload instead (the scan alone) and
            # call once with room for it plus deflate's worst case; a member that is larger still goes the two-call way.
            n = C.c_size_t()
            _check(_L.gs_gaussians_buffer_export_spz_decompressed(*args, None, None, 0, C.byref(n)))
            out = np.empty(n.value + n.value // 8 + 1024, dtype=np.uint8)
            status = _L.gs_gaussians_buffer_write(*head, _ptr(out), out.size, C.byref(n))
            if status == 0 or n.value <= out.size:
                _check(status)
                return out[:n.value].tobytes()
        return _sized_call(_L.gs_gaussians_buffer_write, *head)

    def write_to_file(self, path, stream=None, selection=None, invert=False, fast=False, decompose=False):
        """write() into a file; the format follows the suffix: .spz is SPZ, everything else PLY"""
        source = GaussiansSource.Spz if str(path).lower().endswith(".spz") else GaussiansSource.Ply
        data = self.write(stream, source, selection, invert, fast=fast, decompose=decompose)
        with open(path, "wb") as f:
            f.write(data)

    def snapshot(self, stream, selection=None):
        """gs_gaussians_buffer_snapshot: a Snapshot of the records of `selection` (None: all), the undo
        entry of an edit.  Blocking (the host sizes the allocation from the count); the snapshot keeps its own mask."""
        if selection is not None and not isinstance(selection, Selection):
            raise TypeError("selection must be a Selection or None, not %s" % type(selection).__name__)
        h = C.c_void_p()
        _check(_L.gs_gaussians_buffer_snapshot(self._h, stream._h if stream is not None else None,
                                               selection._h if selection is not None else None, C.byref(h)))
        return Snapshot(self.device, self.pod, h)

    def restore(self, stream, snapshot, exchange=False):
        """gs_gaussians_buffer_restore: writes the snapshot's records back to the indices they came from (this buffer, or
        any buffer of the same layout and length).  Only enqueues, like edit().  exchange=True swaps instead: the snapshot
        then holds what the buffer held — undo is an exchange, redo the same exchange again."""
        if not isinstance(snapshot, Snapshot):
            raise TypeError("snapshot must be a Snapshot, not %s" % type(snapshot).__name__)
        if snapshot._h is None:
            raise ValueError("the snapshot was destroyed")
        _check(_L.gs_gaussians_buffer_restore(self._h, stream._h if stream is not None else None, snapshot._h,
                                              int(bool(exchange))))

    @staticmethod
    def concat(stream, buffers, selections=None, pod=None):
        """gs_gaussians_buffer_create_concat: (a new GaussiansBuffer with the records of selections[i] of buffers[i], one
        source after the other in caller order, counts per source).  selections=None, or None for a source: all of it.
        The same buffer may be given more than once.  Blocks once, for the counts; the copies are enqueued on the stream.
        pod=None: the sources share one layout.  pod=a GaussianPod: gs_gaussians_buffer_create_concat_as — the sources may
        have any layouts and each is converted to `pod`; LossyConfigError if one cannot be."""
        if pod is not None and not isinstance(pod, GaussianPod):
            raise TypeError("pod must be a GaussianPod or None, not %s" % type(pod).__name__)
        buffers = list(buffers)
        for b in buffers:
            if not isinstance(b, GaussiansBuffer):
                raise TypeError("buffers must be GaussiansBuffers, not %s" % type(b).__name__)
        sels = [None] * len(buffers) if selections is None else list(selections)
        if len(sels) != len(buffers):
            raise ValueError("%d selections for %d buffers" % (len(sels), len(buffers)))
        for sel in sels:
            if sel is not None and not isinstance(sel, Selection):
                raise TypeError("selections must be Selections or None, not %s" % type(sel).__name__)
        k = len(buffers)
        src = (C.c_void_p * k)(*[b._h for b in buffers])
        sel = (C.c_void_p * k)(*[x._h if x is not None else None for x in sels])
        counts, h = (C.c_uint64 * k)(), C.c_void_p()
        st = stream._h if stream is not None else None
        if pod is None:
            _check(_L.gs_gaussians_buffer_create_concat(st, src, sel, k, C.byref(h), counts))
        else:
            _check(_L.gs_gaussians_buffer_create_concat_as(st, src, sel, k, pod.sh, pod.cov, C.byref(h), counts))
        # (no buffer, more than 64, or two layouts: the library's GS_ERR_INVALID_ARGUMENT above)
        return GaussiansBuffer(buffers[0].device, buffers[0].pod if pod is None else pod, h), [int(c) for c in counts]

    def stats(self, stream, selection=None, model_transform=None, ref=(0.0, 0.0, 0.0)):
        """gs_gaussians_buffer_stats: a GaussianStats — count and, for each of the nine ATTR_*, the number
        of finite values, their bit-defined min and max and their binary64 sum — over the records of `selection` (None:
        all), in one pass on the device.  Blocking.  model_transform=None: the default transform; `ref` is the reference
        point of ATTR_DIST2."""
        if selection is not None and not isinstance(selection, Selection):
            raise TypeError("selection must be a Selection or None, not %s" % type(selection).__name__)
        if model_transform is not None and not isinstance(model_transform, ModelTransformPod):
            raise TypeError("model_transform must be a ModelTransformPod or None, not %s" % type(model_transform).__name__)
        r = (C.c_float * 3)(*_ref_point(ref))
        out = _capi.Stats()
        _check(_L.gs_gaussians_buffer_stats(self._h, stream._h if stream is not None else None,
                                            selection._h if selection is not None else None,
                                            C.byref(model_transform) if model_transform is not None else None, r, C.byref(out)))
        a = out.attr
        return GaussianStats(count=int(out.count),
                             finite=np.array([a[k].finite for k in range(ATTR_COUNT)], np.uint64),
                             min=np.array([a[k].min for k in range(ATTR_COUNT)], np.float32),
                             max=np.array([a[k].max for k in range(ATTR_COUNT)], np.float32),
                             sum=np.array([a[k].sum for k in range(ATTR_COUNT)], np.float64))

    def histogram(self, stream, attr, lo, hi, bins, selection=None, model_transform=None, ref=(0.0, 0.0, 0.0)):
        """gs_gaussians_buffer_histogram: np.uint64[2, bins + 3] — row 0 the Gaussians of `selection`
        (None: all of them), row 1 the others; columns 0..bins-1 the bins of [lo, hi), then below, above and NaN.
        Blocking.  `attr`: an ATTR_* number or its name."""
        if selection is not None and not isinstance(selection, Selection):
            raise TypeError("selection must be a Selection or None, not %s" % type(selection).__name__)
        d = attribute_desc(attr, model_transform, ref)
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)):
            raise TypeError("bins must be an integer, not %s" % type(bins).__name__)
        if not 1 <= int(bins) <= 4096:
            raise ValueError("a histogram takes 1 to 4096 bins, not %d" % bins)
        out = np.zeros((2, int(bins) + 3), dtype=np.uint64)
        _check(_L.gs_gaussians_buffer_histogram(self._h, stream._h if stream is not None else None,
                                                selection._h if selection is not None else None, C.byref(d), float(lo), float(hi),
                                                int(bins), _ptr(out)))
        return out

    def neighbor_counts(self, stream, radius, cap=NEIGHBOR_COUNT_MAX, among=None, model_transform=None, out=None):
        """gs_gaussians_buffer_neighbor_counts: a Buffer of one uint32 per Gaussian in caller order,
        min(c_i, cap), c_i = the Gaussians of `among` (None: all) with a finite world position within `radius` of Gaussian i,
        itself not counted; 0 where i is not in `among` or has no finite position.  Only enqueues; read the plane with
        Buffer.download(stream, np.uint32).  `out`: a Buffer of at least 4 len() bytes to write into instead of a new one.
        A small `cap` bounds the cost where the scene is dense."""
        radius, among, mt = _neighbor_args(radius, among, model_transform)
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)):
            raise TypeError("cap must be an integer, not %s" % type(cap).__name__)
        if not 1 <= int(cap) <= NEIGHBOR_COUNT_MAX:
            raise ValueError("cap must be between 1 and 2^32 - 1, not %d" % cap)
        if out is not None and not isinstance(out, Buffer):
            raise TypeError("out must be a Buffer or None, not %s" % type(out).__name__)
        own = out is None
        if own:
            out = Buffer(self.device, size=max(4 * self.len(), 4))
        try:
            _check(_L.gs_gaussians_buffer_neighbor_counts(self._h, stream._h if stream is not None else None, among, mt, radius,
                                                          int(cap), out._h))
        except Exception:
            if own:
                out.release()
            raise
        return out

    def components(self, stream, radius, among=None, model_transform=None, labels_out=None, sizes_out=None, info_out=None):
        """gs_gaussians_buffer_components: the connected components of the neighbour graph within
        `radius` (points and neighbours as in neighbor_counts).  Returns three Buffers (labels, sizes, info): one uint32 per
        Gaussian in caller order with the smallest index of its component (COMPONENT_NONE where it is no point), one with
        the number of points of its component (0 where it is no point), and 16 bytes of COMPONENTS_INFO_DTYPE.  Only
        enqueues; read them with Buffer.download.  A Buffer that is not given is allocated (and released again if the call
        fails); one that is given holds at least 4 len() bytes (16 for the info)."""
        radius, among, mt = _neighbor_args(radius, among, model_transform)
        outs = [labels_out, sizes_out, info_out]
        for name, b in zip(("labels_out", "sizes_out", "info_out"), outs):
            if b is not None and not isinstance(b, Buffer):
                raise TypeError("%s must be a Buffer or None, not %s" % (name, type(b).__name__))
        own = []
        try:
            for k, size in enumerate((max(4 * self.len(), 4), max(4 * self.len(), 4), 16)):
                if outs[k] is None:
                    outs[k] = Buffer(self.device, size=size)
                    own.append(outs[k])
            _check(_L.gs_gaussians_buffer_components(self._h, stream._h if stream is not None else None, among, mt, radius,
                                                     outs[0]._h, outs[1]._h, outs[2]._h))
        except Exception:
            for b in own:
                b.release()
            raise
        return tuple(outs)

    def simplify(self, stream, cell_size, pod=None, among=None, cell_of_out=None):
        """gs_gaussians_buffer_create_simplified: a new GaussiansBuffer of layout `pod` (None: this
        buffer's; every layout is a valid target) in which the Gaussians of `among` (None: all) that share a grid cell of
        side `cell_size` on their stored positions are merged into one — opacity x size weighted mean, second moments about
        the cell centre, opacity x size mass kept — in ascending cell order; a Gaussian alone in its cell is converted bit for
        bit.  Blocking.  cell_of_out: True for a new Buffer, or a Buffer of at least 4 len() bytes; then (buffer, cell_of) is
        returned and word i of the plane is the record Gaussian i went into, 0xffffffff where it is not in `among` or has no
        finite position."""
        cell_size, among, _ = _neighbor_args(cell_size, among, None)
        pod = self.pod if pod is None else pod
        if not isinstance(pod, GaussianPod):
            raise TypeError("pod must be a GaussianPod or None, not %s" % type(pod).__name__)
        own = cell_of_out is True
        if own:
            cell_of_out = Buffer(self.device, size=max(4 * self.len(), 4))
        elif cell_of_out is not None and not isinstance(cell_of_out, Buffer):
            raise TypeError("cell_of_out must be a Buffer, True or None, not %s" % type(cell_of_out).__name__)
        h, count = C.c_void_p(), C.c_uint64()
        try:
            _check(_L.gs_gaussians_buffer_create_simplified(self._h, stream._h if stream is not None else None, among, cell_size,
                                                            pod.sh, pod.cov, cell_of_out._h if cell_of_out is not None else None,
                                                            C.byref(h), C.byref(count)))
        except Exception:
            if own:
                cell_of_out.release()
            raise
        out = GaussiansBuffer(self.device, pod, h)
        assert out.len() == count.value
        return out if cell_of_out is None else (out, cell_of_out)

    def knn(self, stream, k, radius, among=None, queries=None, model_transform=None, dist2_out=None, index_out=None,
            indices=False):
        """gs_gaussians_buffer_knn: a Buffer of k binary32 values per Gaussian in caller order, row i at
        i k: the squared distances from Gaussian i to its k nearest other Gaussians of `among` (None: all) within `radius`,
        ascending, ties to the smaller index, padded with +inf where fewer than k lie within the radius; all NaN where i is
        not in `among` or has no finite world position.  indices=True (or an index_out Buffer): (dist2, index) is returned,
        the second plane holding the uint32 indices of those neighbours, KNN_NONE in the padding.  `queries` (a Selection;
        None: all) names the rows that are written: every other row of a Buffer that is given keeps its bytes.  Only
        enqueues; read the planes with Buffer.download.  A Buffer that is given holds at least 4 k len() bytes."""
        k = _knn_k(k)
        radius, among, mt = _neighbor_args(radius, among, model_transform)
        if queries is not None and not isinstance(queries, Selection):
            raise TypeError("queries must be a Selection or None, not %s" % type(queries).__name__)
        for name, b in (("dist2_out", dist2_out), ("index_out", index_out)):
            if b is not None and not isinstance(b, Buffer):
                raise TypeError("%s must be a Buffer or None, not %s" % (name, type(b).__name__))
        if not isinstance(indices, bool):
            raise TypeError("indices must be a bool, not %s" % type(indices).__name__)
        own = []
        try:
            if dist2_out is None:
                dist2_out = Buffer(self.device, size=max(4 * k * self.len(), 4))
                own.append(dist2_out)
            if index_out is None and indices:
                index_out = Buffer(self.device, size=max(4 * k * self.len(), 4))
                own.append(index_out)
            _check(_L.gs_gaussians_buffer_knn(self._h, stream._h if stream is not None else None, among,
                                              queries._h if queries is not None else None, mt, k, radius, dist2_out._h,
                                              index_out._h if index_out is not None else None))
        except Exception:
            for b in own:
                b.release()
            raise
        return dist2_out if index_out is None else (dist2_out, index_out)

    def knn_auto(self, stream, k, among=None, model_transform=None, radius0=None, max_passes=24):
        """The k-NN rows without a radius guess: (dist2, index, radius, passes).  A host policy over knn, select_knn and
        Selection.count (not normative): the bounds and the point count come from stats(); the first pass
        writes every row at radius0 (None: half the largest extent times (k / points)^(1/3)); while rows are incomplete,
        the radius is below the diagonal of the bounding box and passes remain, the radius doubles and the incomplete rows
        alone are searched again.  A complete row is the same at every larger radius, so the planes equal those of one knn
        call at the returned radius bit for bit.  Blocks once per pass (the count of incomplete rows)."""
        k = _knn_k(k)
        if not isinstance(stream, Stream):
            raise TypeError("stream must be a Stream, not %s" % type(stream).__name__)
        _neighbor_args(0.0, among, model_transform)
        if isinstance(max_passes, bool) or not isinstance(max_passes, (int, np.integer)):
            raise TypeError("max_passes must be an integer, not %s" % type(max_passes).__name__)
        if int(max_passes) < 1:
            raise ValueError("max_passes must be at least 1, not %d" % max_passes)
        if radius0 is not None:
            radius0 = np.float32(_neighbor_args(radius0, None, None)[0])
        st = self.stats(stream, selection=among, model_transform=model_transform)
        points = int(st.finite[:3].min())
        lo, hi = st.bounds
        ext = (hi.astype(np.float64) - lo.astype(np.float64)) if points else np.zeros(3)
        diagonal = float(np.sqrt((ext * ext).sum()))
        limit = np.float32(1.8e19)      # the largest radius whose binary32 square is finite, rounded down
        if radius0 is None:
            radius0 = np.float32(min(0.5 * float(ext.max()) * (k / points) ** (1.0 / 3.0), float(limit))) if points else np.float32(0.0)
        radius, n = radius0, self.len()
        dist2, index = self.knn(stream, k, float(radius), among=among, model_transform=model_transform, indices=True)
        passes, todo = 1, None
        try:
            while passes < int(max_passes) and float(radius) < diagonal and radius < limit:
                if todo is None:
                    todo = Selection(self.device, n)
                todo.select_knn(stream, dist2, k, KNN_KTH_DIST2, float("inf"), float("inf"))
                if not todo.count(stream):
                    break
                radius = min(radius * np.float32(2.0), limit) if radius > 0 else np.float32(min(diagonal * 2.0 ** -10, float(limit)))
                self.knn(stream, k, float(radius), among=among, queries=todo, model_transform=model_transform, dist2_out=dist2,
                         index_out=index)
                passes += 1
            stream.synchronize()
        except Exception:
            dist2.release()
            index.release()
            raise
        finally:
            if todo is not None:
                stream.synchronize()
                todo.destroy()
        return dist2, index, float(radius), passes

    def _between_args(self, target, queries, among, model_transform, target_transform):
        """the arguments the calls between two buffers share, checked before any library call"""
        if not isinstance(target, GaussiansBuffer):
            raise TypeError("target must be a GaussiansBuffer, not %s" % type(target).__name__)
        if target is self:
            raise ValueError("target is this buffer: that is knn()")
        for name, v in (("queries", queries), ("among", among)):
            if v is not None and not isinstance(v, Selection):
                raise TypeError("%s must be a Selection or None, not %s" % (name, type(v).__name__))
        for name, v in (("model_transform", model_transform), ("target_transform", target_transform)):
            if v is not None and not isinstance(v, ModelTransformPod):
                raise TypeError("%s must be a ModelTransformPod or None, not %s" % (name, type(v).__name__))

    def knn_to(self, stream, target, k, radius, queries=None, among=None, model_transform=None, target_transform=None,
               dist2_out=None, index_out=None, indices=False):
        """gs_gaussians_buffer_knn_between: a Buffer of k binary32 values per Gaussian of THIS buffer in
        caller order, row i at i k: the squared distances from Gaussian i (under model_transform) to its k nearest Gaussians
        of `target` (another GaussiansBuffer, under target_transform; `among`, a Selection of the target, None: all) within
        `radius`, ascending, ties to the smaller target index, padded with +inf; all NaN where i has no finite world
        position.  indices=True (or an index_out Buffer): (dist2, index), the second plane holding the uint32 TARGET indices,
        KNN_NONE in the padding.  `queries` (a Selection of this buffer; None: all) names the rows that are written.  Only
        enqueues; the planes are those of knn(): select_knn and knn_summary take them with n = self.len()."""
        k = _knn_k(k)
        radius, _, _ = _neighbor_args(radius, None, None)
        self._between_args(target, queries, among, model_transform, target_transform)
        for name, b in (("dist2_out", dist2_out), ("index_out", index_out)):
            if b is not None and not isinstance(b, Buffer):
                raise TypeError("%s must be a Buffer or None, not %s" % (name, type(b).__name__))
        if not isinstance(indices, bool):
            raise TypeError("indices must be a bool, not %s" % type(indices).__name__)
        own = []
        try:
            if dist2_out is None:
                dist2_out = Buffer(self.device, size=max(4 * k * self.len(), 4))
                own.append(dist2_out)
            if index_out is None and indices:
                index_out = Buffer(self.device, size=max(4 * k * self.len(), 4))
                own.append(index_out)
            _check(_L.gs_gaussians_buffer_knn_between(
                self._h, target._h, stream._h if stream is not None else None, queries._h if queries is not None else None,
                among._h if among is not None else None, C.byref(model_transform) if model_transform is not None else None,
                C.byref(target_transform) if target_transform is not None else None, k, radius, dist2_out._h,
                index_out._h if index_out is not None else None))
        except Exception:
            for b in own:
                b.release()
            raise
        return dist2_out if index_out is None else (dist2_out, index_out)

    def pair_sums(self, stream, target, index_plane, k=1, queries=None, model_transform=None, target_transform=None):
        """gs_gaussians_buffer_pair_sums: the PairSums over the pairs (Gaussian i of this buffer, Gaussian
        index_plane[i k] of `target`) for the i of `queries` (the Selection given to knn_to, or a subset; None: all) — an
        index at or beyond target.len() names no pair and is never followed.  Blocking; the same bits from run to run."""
        k = _knn_k(k)
        self._between_args(target, queries, None, model_transform, target_transform)
        if not isinstance(index_plane, Buffer):
            raise TypeError("index_plane must be a Buffer, not %s" % type(index_plane).__name__)
        out = _capi.PairSumsRecord()
        _check(_L.gs_gaussians_buffer_pair_sums(
            self._h, target._h, stream._h if stream is not None else None, queries._h if queries is not None else None,
            C.byref(model_transform) if model_transform is not None else None,
            C.byref(target_transform) if target_transform is not None else None, index_plane._h, k, C.byref(out)))
        return PairSums.from_record(out)

    def chamfer_to(self, stream, target, radius, model_transform=None, target_transform=None):
        """The two-sided Chamfer distance to `target` within `radius`, without a download of the planes: a Chamfer of the mean
        nearest-neighbour distance from this buffer to the target and back, over the Gaussians that have a neighbour within
        the radius, and the numbers that have none (`incomplete`).  Two knn_to calls with k = 1 and two
        knn_summary(KNN_MEAN_DIST) (a host policy).  Blocking."""
        if not isinstance(stream, Stream):
            raise TypeError("stream must be a Stream, not %s" % type(stream).__name__)
        radius, _, _ = _neighbor_args(radius, None, None)
        self._between_args(target, None, None, model_transform, target_transform)
        sides = []
        for a, b, ma, mb in ((self, target, model_transform, target_transform), (target, self, target_transform, model_transform)):
            plane = a.knn_to(stream, b, 1, radius, model_transform=ma, target_transform=mb)
            try:
                sides.append(knn_summary(stream, plane, a.len(), 1, KNN_MEAN_DIST))
            finally:
                stream.synchronize()
                plane.release()
        return Chamfer(to_target=sides[0], from_target=sides[1])

    def align_to(self, stream, target, radius, queries=None, among=None, model_transform=None, target_transform=None, scale=False,
                 max_iterations=32, rms_tol=1e-4):
        """ICP of this buffer onto `target` (a host policy): (pod, report).  Edits nothing: every iteration
        runs knn_to (k = 1, indices) under the current transform — model_transform (None: the default pod) composed with
        the fits so far —, then pair_sums, and, unless it stops, rigid_fit and compose_model_transform.  It stops when the
        RMS of the pairs has not fallen by more than rms_tol of its previous value, or is at most rms_tol x radius
        ('converged'), when there are fewer than 3 pairs ('pairs'), or after max_iterations ('iterations').  pod: the
        ModelTransformPod the last entry of the report was measured under; bake it with edit(TRANSFORM | ROTATE_SH) or
        pass it as the frame's model transform.  report: an AlignReport with one (pairs, rms) per iteration.  Only pairs
        within `radius` count, so the radius is the largest misalignment that can be undone.  `queries` subsamples this
        buffer, `among` the target.  Blocking."""
        if not isinstance(stream, Stream):
            raise TypeError("stream must be a Stream, not %s" % type(stream).__name__)
        radius, _, _ = _neighbor_args(radius, None, None)
        self._between_args(target, queries, among, model_transform, target_transform)
        if not isinstance(scale, bool):
            raise TypeError("scale must be a bool, not %s" % type(scale).__name__)
        if isinstance(max_iterations, bool) or not isinstance(max_iterations, (int, np.integer)):
            raise TypeError("max_iterations must be an integer, not %s" % type(max_iterations).__name__)
        if int(max_iterations) < 1:
            raise ValueError("max_iterations must be at least 1, not %d" % max_iterations)
        if isinstance(rms_tol, bool) or not isinstance(rms_tol, (int, float, np.integer, np.floating)):
            raise TypeError("rms_tol must be a number, not %s" % type(rms_tol).__name__)
        if not (np.isfinite(rms_tol) and rms_tol >= 0):
            raise ValueError("rms_tol must be finite and >= 0, not %r" % (rms_tol,))
        current = model_transform if model_transform is not None else model_transform_pod()
        size = max(4 * self.len(), 4)
        dist2, index = Buffer(self.device, size=size), Buffer(self.device, size=size)
        entries, stopped, previous = [], "iterations", None
        try:
            for it in range(int(max_iterations)):
                self.knn_to(stream, target, 1, radius, queries=queries, among=among, model_transform=current,
                            target_transform=target_transform, dist2_out=dist2, index_out=index)
                sums = self.pair_sums(stream, target, index, 1, queries=queries, model_transform=current,
                                      target_transform=target_transform)
                entries.append((sums.pairs, sums.rms))
                if sums.pairs < 3:
                    stopped = "pairs"
                    break
                if sums.rms <= float(rms_tol) * radius or (previous is not None and not previous - sums.rms > float(rms_tol) * previous):
                    stopped = "converged"
                    break
                if it + 1 == int(max_iterations):
                    break
                delta, _ = rigid_fit(sums, scale)
                current = compose_model_transform(delta, current)
                previous = sums.rms
        finally:
            stream.synchronize()
            dist2.release()
            index.release()
        return current, AlignReport(iterations=entries, stopped=stopped)

    def destroy(self):
        if self._h:
            _L.gs_gaussians_buffer_destroy(self._h)
            self._h = None


class GaussianTransformBuffer(Buffer):
    """src/buffer/gaussian_transform.rs:104-163"""

    def __init__(self, device, _handle=None):
        if _handle is None:
            _handle = C.c_void_p()
            _check(_L.gs_gaussian_transform_buffer_create(device._h, C.byref(_handle)))
        super().__init__(device, _handle=_handle)

    @staticmethod
    def try_from(buffer):
        _check(_L.gs_gaussian_transform_buffer_from_buffer(buffer._h))
        return GaussianTransformBuffer(buffer.device, _handle=C.c_void_p(_L.gs_buffer_retain(buffer._h)))

    def update(self, stream, size, display_mode, sh_deg, no_sh0, max_std_dev):
        self.update_with_pod(stream, gaussian_transform_pod(size, display_mode, sh_deg, no_sh0, max_std_dev))

    def update_with_pod(self, stream, pod):
        _check(_L.gs_gaussian_transform_buffer_update(self._h, stream._h, C.byref(pod)))


class ModelTransformBuffer(Buffer):
    """src/buffer/model_transform.rs:10-58"""

    def __init__(self, device, _handle=None):
        if _handle is None:
            _handle = C.c_void_p()
            _check(_L.gs_model_transform_buffer_create(device._h, C.byref(_handle)))
        super().__init__(device, _handle=_handle)

    @staticmethod
    def try_from(buffer):
        _check(_L.gs_model_transform_buffer_from_buffer(buffer._h))
        return ModelTransformBuffer(buffer.device, _handle=C.c_void_p(_L.gs_buffer_retain(buffer._h)))

    def update(self, stream, pos, rot, scale):
        self.update_with_pod(stream, model_transform_pod(pos, rot, scale))

    def update_with_pod(self, stream, pod):
        _check(_L.gs_model_transform_buffer_update(self._h, stream._h, C.byref(pod)))


# ------------------------------------------------------------------------------------------------
# ComputeBundle
# ------------------------------------------------------------------------------------------------

class KernelRegistry:
    """The resolver: maps a module path to a kernel of the built-in library (the HIP analogue of
    wesl::PkgResolver over shader::PACKAGE, src/shader.rs:8-56)."""
    MODULES = {"array_map_add": KERNEL_ARRAY_MAP_ADD, "test_gaussian": KERNEL_TEST_GAUSSIAN,
               "test_gaussian_transform": KERNEL_TEST_GAUSSIAN_TRANSFORM,
               "test_model_transform": KERNEL_TEST_MODEL_TRANSFORM, "unpack_soa": KERNEL_UNPACK_SOA}

    def resolve(self, path):
        key = path.split("::")[-1]
        if key not in self.MODULES:
            raise KernelResolveError("module not found: %s" % path)
        return self.MODULES[key]


class SourceResolver:
    """Resolver over caller-supplied HIP C++ modules (the analogue of a wesl::PkgResolver holding
    the caller's own package next to shader::PACKAGE).  A module's text may
    `#include <wgpu_3dgs_core.h>` to import the device library."""

    def __init__(self, modules=None):
        self.modules = dict(modules or {})

    def add_module(self, path, source):
        self.modules[path] = source
        return self

    def resolve(self, path):
        if path not in self.modules:
            raise KernelResolveError("module not found: %s" % path)
        return self.modules[path]


def _buffer_array(buffers):
    arr = (C.c_void_p * len(buffers))(*[b._h for b in buffers])
    return arr


class ComputeBundle:
    """src/compute_bundle.rs:49-351.  `layouts` = bindings per bind group."""

    def __init__(self, device, handle, managed):
        self.device, self._h, self._managed = device, handle, managed

    @staticmethod
    def _desc(label, kernel, pod, layouts, workgroup_size, constants, keep):
        d = _capi.BundleDesc()
        d.label = label.encode() if label else None
        d.kernel = kernel
        d.sh, d.cov = (pod.sh, pod.cov) if pod is not None else (0, 0)
        d.bind_group_count = len(layouts)
        arr = (C.c_uint32 * max(len(layouts), 1))(*layouts)
        d.bindings_per_group = arr
        d.workgroup_size = workgroup_size or 0
        names = (C.c_char_p * max(len(constants), 1))(*[k.encode() for k in constants])
        vals = (C.c_double * max(len(constants), 1))(*[float(v) for v in constants.values()])
        d.constant_names, d.constant_values, d.constant_count = names, vals, len(constants)
        keep.extend([arr, names, vals])
        return d

    @staticmethod
    def new(label, device, layouts, resources, kernel, pod=None, workgroup_size=None, constants=None):
        """ComputeBundle::new — :141-188"""
        keep = []
        d = ComputeBundle._desc(label, kernel, pod, list(layouts), workgroup_size, constants or {}, keep)
        resources = [list(r) for r in resources]
        groups = [_buffer_array(r) for r in resources]
        gp = (C.c_void_p * max(len(groups), 1))(*[C.cast(g, C.c_void_p) for g in groups])
        counts = (C.c_uint32 * max(len(groups), 1))(*[len(r) for r in resources])
        h = C.c_void_p()
        _check(_L.gs_bundle_create_with_bind_groups(device._h, C.byref(d), gp, counts, len(groups),
                                                    C.byref(h)))
        return ComputeBundle(device, h, True)

    @staticmethod
    def new_without_bind_groups(label, device, layouts, kernel, pod=None, workgroup_size=None,
                                constants=None):
        """ComputeBundle::new_without_bind_groups — :260-341"""
        keep = []
        d = ComputeBundle._desc(label, kernel, pod, list(layouts), workgroup_size, constants or {}, keep)
        h = C.c_void_p()
        _check(_L.gs_bundle_create(device._h, C.byref(d), C.byref(h)))
        return ComputeBundle(device, h, False)

    @staticmethod
    def new_from_source(label, device, layouts, source, entry_point, pod=None, workgroup_size=None,
                        constants=None, defines=(), resources=None):
        """Compile `source` (HIP C++) with hiprtc: ComputeBundleBuilder::build for a custom shader."""
        constants = constants or {}
        d = _capi.BundleSourceDesc()
        d.label = label.encode() if label else None
        d.source = source.encode()
        d.entry_point = entry_point.encode()
        d.sh, d.cov = (pod.sh, pod.cov) if pod is not None else (0, 0)
        layouts = list(layouts)
        arr = (C.c_uint32 * max(len(layouts), 1))(*layouts)
        d.bind_group_count, d.bindings_per_group = len(layouts), arr
        d.workgroup_size = workgroup_size or 0
        names = (C.c_char_p * max(len(constants), 1))(*[k.encode() for k in constants])
        vals = (C.c_double * max(len(constants), 1))(*[float(v) for v in constants.values()])
        d.constant_names, d.constant_values, d.constant_count = names, vals, len(constants)
        defs = (C.c_char_p * max(len(defines), 1))(*[x.encode() for x in defines])
        d.defines, d.define_count = defs, len(defines)
        h = C.c_void_p()
        status = _L.gs_bundle_create_from_source(device._h, C.byref(d), C.byref(h))
        if status == -20:
            info = _capi.ErrorInfo()
            _L.gs_last_error(C.byref(info))
            raise KernelResolveError(info.message.decode(errors="replace"))
        _check(status)
        bundle = ComputeBundle(device, h, False)
        if resources is not None:
            resources = [list(r) for r in resources]
            groups = [_buffer_array(r) for r in resources]
            gp = (C.c_void_p * max(len(groups), 1))(*[C.cast(g, C.c_void_p) for g in groups])
            counts = (C.c_uint32 * max(len(groups), 1))(*[len(r) for r in resources])
            try:
                _check(_L.gs_bundle_attach_bind_groups(h, gp, counts, len(groups)))
            except GsError:
                bundle.destroy()
                raise
            bundle._managed = True
        return bundle

    def workgroup_size(self):
        return _L.gs_bundle_workgroup_size(self._h)

    def label(self):
        v = _L.gs_bundle_label(self._h)
        return v.decode() if v else None

    def bind_group_layouts(self):
        return _L.gs_bundle_bind_group_layout_count(self._h)

    def bind_groups(self):
        return _L.gs_bundle_bind_group_count(self._h)

    def update_bind_group_with_binding_resources(self, index, resources):
        """Returns False when index is out of bounds (Rust: None) — :222-231"""
        if index >= self.bind_groups():
            return False
        resources = list(resources)
        _check(_L.gs_bundle_set_bind_group(self._h, index, _buffer_array(resources), len(resources)))
        return True

    def dispatch(self, stream, count, bind_groups=None):
        """dispatch(encoder, count) / ComputeBundle<()>::dispatch(encoder, count, bind_groups)"""
        if bind_groups is None:
            _check(_L.gs_bundle_dispatch(self._h, stream._h, count))
            return
        bind_groups = [list(g) for g in bind_groups]
        groups = [_buffer_array(g) for g in bind_groups]
        gp = (C.c_void_p * max(len(groups), 1))(*[C.cast(g, C.c_void_p) for g in groups])
        counts = (C.c_uint32 * max(len(groups), 1))(*[len(g) for g in bind_groups])
        _check(_L.gs_bundle_dispatch_with_bind_groups(self._h, stream._h, count, gp, counts, len(groups)))

    def last_workgroup_count(self):
        return _L.gs_bundle_last_workgroup_count(self._h)

    def destroy(self):
        if self._h:
            _L.gs_bundle_destroy(self._h)
            self._h = None


class ComputeBundleBuilder:
    """src/compute_bundle.rs:364-593: same required fields, checked in the same order."""

    def __init__(self):
        self._label = None
        self._layouts = []
        self._constants = {}
        self._entry_point = None
        self._main_shader = None
        self._pod = None
        self._resolver = None
        self._workgroup_size = None
        self._defines = ()

    def label(self, label):
        self._label = label
        return self

    def bind_group_layout(self, bindings):
        """`bindings` = number of entries of the BindGroupLayoutDescriptor"""
        self._layouts.append(int(bindings))
        return self

    def bind_group_layouts(self, layouts):
        self._layouts.extend(int(b) for b in layouts)
        return self

    def pipeline_compile_options(self, constants):
        self._constants = dict(constants)
        return self

    def entry_point(self, name):
        self._entry_point = name
        return self

    def main_shader(self, module_path):
        self._main_shader = module_path
        return self

    def wesl_compile_options(self, features, defines=()):
        """`features` = a GaussianPod (its features() select the kernel instantiation / the
        GS_SH, GS_COV and feature-name macros); `defines` = further feature flags"""
        self._pod = features
        self._defines = tuple(defines)
        return self

    def resolver(self, resolver):
        self._resolver = resolver
        return self

    def workgroup_size(self, n):
        self._workgroup_size = n
        return self

    def _resolve(self):
        if not self._layouts:
            raise MissingBindGroupLayout("missing bind group layout for compute bundle")
        if self._resolver is None:
            raise MissingResolver("missing resolver for compute bundle")
        if self._entry_point is None:
            raise MissingEntryPoint("missing entry point for compute bundle")
        if self._main_shader is None:
            raise MissingMainShader("missing main shader for compute bundle")
        return self._resolver.resolve(self._main_shader)

    def build(self, device, resources):
        kernel = self._resolve()
        if isinstance(kernel, str):   # a module of a SourceResolver: compile it
            return ComputeBundle.new_from_source(self._label, device, self._layouts, kernel,
                                                 self._entry_point, self._pod, self._workgroup_size,
                                                 self._constants, self._defines, resources)
        return ComputeBundle.new(self._label, device, self._layouts, resources, kernel, self._pod,
                                 self._workgroup_size, self._constants)

    def build_without_bind_groups(self, device):
        kernel = self._resolve()
        if isinstance(kernel, str):
            return ComputeBundle.new_from_source(self._label, device, self._layouts, kernel,
                                                 self._entry_point, self._pod, self._workgroup_size,
                                                 self._constants, self._defines, None)
        return ComputeBundle.new_without_bind_groups(self._label, device, self._layouts, kernel,
                                                     self._pod, self._workgroup_size, self._constants)


# ------------------------------------------------------------------------------------------------
# renderer
# ------------------------------------------------------------------------------------------------

FRAME_FLAG_PAIR_OVERFLOW, FRAME_FLAG_SKIPPED, FRAME_FLAG_RANK_FAULT = 1, 2, 4     # gs_frame_result.flags
PICK_NONE = 0xFFFFFFFF     # GS_PICK_NONE: a pixel of the pick plane whose transmittance never crossed the threshold
STAGE_NAMES = ["repack", "preprocess", "scan", "depth_sort", "expand", "tile_sort", "ranges", "blend", "frame"]


SEL_SET, SEL_OR, SEL_AND, SEL_ANDNOT, SEL_XOR = 0, 1, 2, 3, 4      # gs_select_op: dst = dst op src

# GS_ATTR_*: one binary32 value per record
ATTR_X, ATTR_Y, ATTR_Z, ATTR_RED, ATTR_GREEN, ATTR_BLUE, ATTR_OPACITY, ATTR_SIZE2, ATTR_DIST2 = range(9)
ATTR_COUNT = 9
ATTR_NAMES = ["x", "y", "z", "red", "green", "blue", "opacity", "size2", "dist2"]


def attribute(attr):
    """GS_ATTR_* from its number or name (ATTR_NAMES); ValueError for anything else."""
    if isinstance(attr, str):
        if attr.lower() not in ATTR_NAMES:
            raise ValueError("unknown attribute %r (one of %s)" % (attr, ", ".join(ATTR_NAMES)))
        return ATTR_NAMES.index(attr.lower())
    if isinstance(attr, (int, np.integer)) and not isinstance(attr, bool) and 0 <= int(attr) < ATTR_COUNT:
        return int(attr)
    raise ValueError("unknown attribute %r" % (attr,))


def _ref_point(ref):
    r = tuple(float(v) for v in ref)
    if len(r) != 3:
        raise ValueError("ref takes three numbers, got %d" % len(r))
    return r


def attribute_desc(attr, model_transform=None, ref=(0.0, 0.0, 0.0)):
    """The gs_attribute_desc of histogram() / select_attribute(), checked before any device call: a known attribute, a
    ModelTransformPod or None (the default transform), a finite `ref` for ATTR_DIST2."""
    d = AttributeDesc()
    d.attr = attribute(attr)
    if model_transform is not None:
        if not isinstance(model_transform, ModelTransformPod):
            raise TypeError("model_transform must be a ModelTransformPod or None, not %s" % type(model_transform).__name__)
        d.model_transform = C.pointer(model_transform)
        d._keep = model_transform      # the pod stays alive as long as the struct
    r = _ref_point(ref)
    if d.attr == ATTR_DIST2 and not all(np.isfinite(v) for v in r):
        raise ValueError("the reference point of ATTR_DIST2 must be finite")
    d.ref[:] = r
    return d


@dataclasses.dataclass
class GaussianStats:
    """gs_stats: `count` selected Gaussians and, indexed by ATTR_*, the finite values of each attribute, their min and max
    (+inf / -inf without a finite value) and their binary64 sum."""
    count: int
    finite: np.ndarray       # uint64[9]
    min: np.ndarray          # float32[9]
    max: np.ndarray          # float32[9]
    sum: np.ndarray          # float64[9]

    @property
    def centroid(self):
        """sum / finite of X, Y, Z (NaN where no value is finite)"""
        with np.errstate(all="ignore"):
            return self.sum[:3] / self.finite[:3].astype(np.float64)

    @property
    def bounds(self):
        """(min, max) of X, Y, Z"""
        return self.min[:3].copy(), self.max[:3].copy()
_SELECT_OPS = {"set": SEL_SET, "or": SEL_OR, "and": SEL_AND, "andnot": SEL_ANDNOT, "xor": SEL_XOR}


def select_op(op):
    """gs_select_op from its number or name ('set', 'or', 'and', 'andnot', 'xor'); ValueError for anything else."""
    if isinstance(op, str):
        if op.lower() not in _SELECT_OPS:
            raise ValueError("unknown select op %r (one of %s)" % (op, ", ".join(_SELECT_OPS)))
        return _SELECT_OPS[op.lower()]
    if isinstance(op, (int, np.integer)) and not isinstance(op, bool) and SEL_SET <= int(op) <= SEL_XOR:
        return int(op)
    raise ValueError("unknown select op %r" % (op,))


def selection_words(n):
    """words of an n-bit selection: ceil(n / 32)"""
    if int(n) < 0:
        raise ValueError("a selection cannot have %d bits" % n)
    return (int(n) + 31) // 32


def frame_selection(hide=None, tint=None, tint_rgba=None):
    """The gs_frame_selection of Renderer.render's keywords, or None for the plain frame.  Checked here, before any
    device call: hide / tint must be Selections, tint_rgba goes with tint (four numbers: a finite colour, 0 <= a <= 1)."""
    for name, sel in (("hide", hide), ("tint", tint)):
        if sel is not None and not isinstance(sel, Selection):
            raise TypeError("%s must be a Selection or None, not %s" % (name, type(sel).__name__))
    if tint is None:
        if tint_rgba is not None:
            raise ValueError("tint_rgba without a tint selection")
        if hide is None:
            return None
        rgba = (0.0, 0.0, 0.0, 0.0)
    else:
        if tint_rgba is None:
            raise ValueError("a tint selection needs tint_rgba")
        rgba = tuple(float(v) for v in tint_rgba)
        if len(rgba) != 4:
            raise ValueError("tint_rgba takes four numbers (r, g, b, a), got %d" % len(rgba))
        if not all(np.isfinite(v) for v in rgba[:3]) or not 0.0 <= rgba[3] <= 1.0:
            raise ValueError("tint_rgba: the colour must be finite and the alpha in [0, 1]")
    fs = FrameSelection()
    fs.hide = hide._h if hide is not None else None
    fs.tint = tint._h if tint is not None else None
    fs.tint_rgba[:] = rgba
    fs._keep = (hide, tint)       # the handles stay alive as long as the struct
    return fs


class Selection:
    """gs_selection: one bit per Gaussian of a buffer, in the caller's index order, on the device.
    Every call but download / count only enqueues on the stream."""

    def __init__(self, device, n):
        selection_words(n)
        h = C.c_void_p()
        _check(_L.gs_selection_create(device._h, int(n), C.byref(h)))
        self._h, self.device = h, device

    def __len__(self):
        return _L.gs_selection_len(self._h)

    def clear(self, stream):
        _check(_L.gs_selection_clear(self._h, stream._h))

    def fill(self, stream):
        _check(_L.gs_selection_fill(self._h, stream._h))

    def invert(self, stream):
        _check(_L.gs_selection_invert(self._h, stream._h))

    def combine(self, stream, op, src):
        """self = self op src"""
        if not isinstance(src, Selection):
            raise TypeError("src must be a Selection")
        _check(_L.gs_selection_combine(self._h, stream._h, select_op(op), src._h))

    def count(self, stream):
        out = C.c_uint64()
        _check(_L.gs_selection_count(self._h, stream._h, C.byref(out)))
        return out.value

    def upload(self, stream, bits):
        """bits: a bool array of len(self), or the ceil(n / 32) packed uint32 words"""
        a = np.asarray(bits)
        if a.dtype == np.bool_:
            if a.shape != (len(self),):
                raise ValueError("%d flags for a selection of %d bits" % (a.size, len(self)))
            a = np.packbits(a, bitorder="little")
            a = np.concatenate([a, np.zeros(-len(a) % 4, np.uint8)]).view(np.uint32)
        a = np.ascontiguousarray(a, dtype=np.uint32)
        _check(_L.gs_selection_upload(self._h, stream._h, _ptr(a), len(a)))

    def download_words(self, stream):
        w = np.zeros(selection_words(len(self)), dtype=np.uint32)
        _check(_L.gs_selection_download(self._h, stream._h, _ptr(w), len(w)))
        return w

    def download(self, stream):
        """the selection as a bool array of len(self) (blocking)"""
        w = self.download_words(stream)
        return np.unpackbits(w.view(np.uint8), bitorder="little")[:len(self)].astype(np.bool_)

    def select_sphere(self, stream, gaussians, model_transform, center, radius, op=SEL_SET):
        """self = self op {Gaussians whose world position lies within `radius` of `center`} (gs_select_sphere)"""
        c = (C.c_float * 3)(*[float(v) for v in center])
        _check(_L.gs_select_sphere(self._h, stream._h, gaussians._h, C.byref(model_transform), c, float(radius),
                                   select_op(op)))

    def select_box(self, stream, gaussians, model_transform, world_to_box, op=SEL_SET):
        """self = self op {Gaussians inside the unit box of `world_to_box`, a 3 x 4 matrix given as 12 numbers in
        column-major order} (gs_select_box)"""
        b = np.ascontiguousarray(world_to_box, dtype=np.float32).reshape(-1)
        if b.size != 12:
            raise ValueError("world_to_box takes 12 numbers (3 x 4, column-major)")
        _check(_L.gs_select_box(self._h, stream._h, gaussians._h, C.byref(model_transform), _ptr(b), select_op(op)))

    def select_range(self, stream, start, count, op=SEL_SET):
        """self = self op {i : start <= i < start + count} (gs_select_range); only enqueues.  After GaussiansBuffer.concat
        this is how the pasted part becomes the selection."""
        for name, v in (("start", start), ("count", count)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError("%s must be an integer, not %s" % (name, type(v).__name__))
            if int(v) < 0:
                raise ValueError("%s must be >= 0, not %d" % (name, v))
        op = select_op(op)
        _check(_L.gs_select_range(self._h, stream._h, int(start), int(count), op))

    def select_attribute(self, stream, gaussians, attr, lo, hi, op=SEL_SET, model_transform=None, ref=(0.0, 0.0, 0.0)):
        """self = self op {i : lo <= v_i <= hi}, v = the attribute `attr` (an ATTR_* number or name) of record i of
        `gaussians` (gs_select_attribute); only enqueues.  NaN values are never selected; infinite
        bounds are allowed, NaN bounds are not."""
        if not isinstance(gaussians, GaussiansBuffer):
            raise TypeError("gaussians must be a GaussiansBuffer, not %s" % type(gaussians).__name__)
        d = attribute_desc(attr, model_transform, ref)
        lo, hi = float(lo), float(hi)
        if lo != lo or hi != hi:
            raise ValueError("a bound of the range is NaN")
        op = select_op(op)
        _check(_L.gs_select_attribute(self._h, stream._h, gaussians._h, C.byref(d), lo, hi, op))

    def select_neighbors(self, stream, gaussians, radius, min_count=0, max_count=NEIGHBOR_COUNT_MAX, among=None,
                         model_transform=None, op=SEL_SET):
        """self = self op {i : min_count <= c_i <= max_count}, c_i = the neighbour count of Gaussian i of `gaussians` within
        `radius` (gs_select_neighbors; see GaussiansBuffer.neighbor_counts); only enqueues.
        max_count = k - 1 selects the floaters with fewer than k others around them.  A Gaussian outside `among` or without
        a finite world position is never selected; min_count > max_count selects nothing."""
        if not isinstance(gaussians, GaussiansBuffer):
            raise TypeError("gaussians must be a GaussiansBuffer, not %s" % type(gaussians).__name__)
        radius, among, mt = _neighbor_args(radius, among, model_transform)
        for name, v in (("min_count", min_count), ("max_count", max_count)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError("%s must be an integer, not %s" % (name, type(v).__name__))
            if not 0 <= int(v) <= NEIGHBOR_COUNT_MAX:
                raise ValueError("%s must be between 0 and 2^32 - 1, not %d" % (name, v))
        op = select_op(op)
        _check(_L.gs_select_neighbors(self._h, stream._h if stream is not None else None, gaussians._h, among, mt, radius,
                                      int(min_count), int(max_count), op))

    def select_components(self, stream, gaussians, radius, min_size=1, max_size=NEIGHBOR_COUNT_MAX, among=None,
                          model_transform=None, op=SEL_SET):
        """self = self op {i : min_size <= S_i <= max_size}, S_i = the number of points in the connected component of Gaussian
        i of `gaussians` within `radius` (gs_select_components; see GaussiansBuffer.components); only
        enqueues.  max_size = m - 1 selects every cluster smaller than m.  A Gaussian outside `among` or without a finite
        world position is never selected; min_size > max_size selects nothing."""
        if not isinstance(gaussians, GaussiansBuffer):
            raise TypeError("gaussians must be a GaussiansBuffer, not %s" % type(gaussians).__name__)
        radius, among, mt = _neighbor_args(radius, among, model_transform)
        for name, v in (("min_size", min_size), ("max_size", max_size)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError("%s must be an integer, not %s" % (name, type(v).__name__))
            if not 0 <= int(v) <= NEIGHBOR_COUNT_MAX:
                raise ValueError("%s must be between 0 and 2^32 - 1, not %d" % (name, v))
        op = select_op(op)
        _check(_L.gs_select_components(self._h, stream._h if stream is not None else None, gaussians._h, among, mt, radius,
                                       int(min_size), int(max_size), op))

    def select_connected(self, stream, gaussians, radius, seeds, among=None, model_transform=None, op=SEL_SET):
        """self = self op {i : the connected component of Gaussian i within `radius` holds a Gaussian of `seeds`}
        (gs_select_connected); only enqueues.  `seeds` is a Selection of the buffer's length and may be
        `self`, which grows a selection to whole clusters; a picked index becomes a seed through select_range(idx, 1)."""
        if not isinstance(gaussians, GaussiansBuffer):
            raise TypeError("gaussians must be a GaussiansBuffer, not %s" % type(gaussians).__name__)
        radius, among, mt = _neighbor_args(radius, among, model_transform)
        if not isinstance(seeds, Selection):
            raise TypeError("seeds must be a Selection, not %s" % type(seeds).__name__)
        op = select_op(op)
        _check(_L.gs_select_connected(self._h, stream._h if stream is not None else None, gaussians._h, among, mt, radius,
                                      seeds._h, op))

    def select_knn(self, stream, dist2_plane, k, kind, lo, hi, op=SEL_SET):
        """self = self op {i : row i is a point's and lo <= v_i <= hi}, v = the statistic `kind` (KNN_KTH_DIST2: the k-th
        squared distance; KNN_MEAN_DIST: the mean distance to the k neighbours; or their names) of row i of `dist2_plane`, a
        Buffer of len(self) rows of k values that GaussiansBuffer.knn filled (gs_select_knn); only
        enqueues.  v of an incomplete row is +inf: lo = hi = inf selects exactly those.  A NaN row is never selected;
        infinite bounds are allowed, NaN bounds are not; lo > hi selects nothing."""
        if not isinstance(dist2_plane, Buffer):
            raise TypeError("dist2_plane must be a Buffer, not %s" % type(dist2_plane).__name__)
        k, kind = _knn_k(k), knn_kind(kind)
        for name, v in (("lo", lo), ("hi", hi)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise TypeError("%s must be a number, not %s" % (name, type(v).__name__))
        lo, hi = float(lo), float(hi)
        if lo != lo or hi != hi:
            raise ValueError("a bound of the range is NaN")
        op = select_op(op)
        _check(_L.gs_select_knn(self._h, stream._h if stream is not None else None, dist2_plane._h, k, kind, lo, hi, op))

    def select_near(self, stream, gaussians, target, radius, among=None, model_transform=None, target_transform=None, op=SEL_SET):
        """self = self op {i : Gaussian i of `gaussians` has a Gaussian of `target` within `radius`}: the overlap of two
        scans (a host policy).  knn_to with k = 1, then select_knn(KNN_KTH_DIST2, 0, r r): a row without a
        neighbour is +inf, a Gaussian without a finite world position NaN, and neither is selected.  `among`: a Selection of
        the target.  len(self) == gaussians.len().  Blocking."""
        if not isinstance(stream, Stream):
            raise TypeError("stream must be a Stream, not %s" % type(stream).__name__)
        if not isinstance(gaussians, GaussiansBuffer):
            raise TypeError("gaussians must be a GaussiansBuffer, not %s" % type(gaussians).__name__)
        radius, _, _ = _neighbor_args(radius, None, None)
        gaussians._between_args(target, None, among, model_transform, target_transform)
        op = select_op(op)
        if len(self) != gaussians.len():
            raise ValueError("the selection has %d bits, the buffer %d Gaussians" % (len(self), gaussians.len()))
        dist2 = gaussians.knn_to(stream, target, 1, radius, among=among, model_transform=model_transform, target_transform=target_transform)
        try:
            rr = np.float32(radius) * np.float32(radius)
            self.select_knn(stream, dist2, 1, KNN_KTH_DIST2, 0.0, float(rr), op)
        finally:
            stream.synchronize()
            dist2.release()

    def select_statistical_outliers(self, stream, gaussians, k=8, sigma=2.0, among=None, model_transform=None, op=SEL_SET,
                                    radius0=None, max_passes=24):
        """self = self op {the statistical outliers of `gaussians`}: (threshold, radius).  The filter of PCL / Open3D as a
        host policy over GaussiansBuffer.knn_auto, knn_summary and select_knn (not normative): v_i = the
        mean distance from Gaussian i to its k nearest neighbours, threshold = mean + sigma std of v over the complete rows
        in binary64, and every Gaussian with v_i > threshold is selected — a row that is still incomplete at the radius
        knn_auto ended with has v = +inf and is an outlier too.  Gaussians outside `among` or without a finite world
        position are never selected.  Blocking."""
        if not isinstance(gaussians, GaussiansBuffer):
            raise TypeError("gaussians must be a GaussiansBuffer, not %s" % type(gaussians).__name__)
        k = _knn_k(k)
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)):
            raise TypeError("sigma must be a number, not %s" % type(sigma).__name__)
        if not np.isfinite(sigma):
            raise ValueError("sigma must be finite, not %r" % (sigma,))
        op = select_op(op)
        if len(self) != gaussians.len():
            raise ValueError("the selection has %d bits, the buffer %d Gaussians" % (len(self), gaussians.len()))
        dist2, index, radius, _ = gaussians.knn_auto(stream, k, among=among, model_transform=model_transform, radius0=radius0,
                                                     max_passes=max_passes)
        try:
            s = knn_summary(stream, dist2, len(self), k, KNN_MEAN_DIST)
            threshold = s.mean + float(sigma) * s.std if s.complete else float("inf")
            # the smallest binary32 above the threshold: the range of select_knn is closed
            with np.errstate(over="ignore"):
                lo = np.float32(threshold)
            if float(lo) <= threshold:
                lo = np.nextafter(lo, np.float32(np.inf))
            self.select_knn(stream, dist2, k, KNN_MEAN_DIST, float(lo), float("inf"), op)
            stream.synchronize()
        finally:
            dist2.release()
            index.release()
        return threshold, radius

    def destroy(self):
        if self._h:
            _L.gs_selection_destroy(self._h)
            self._h = None


# GS_CONTRIB_*: the value gs_select_contribution compares
CONTRIB_SUM, CONTRIB_HITS, CONTRIB_MAX = 0, 1, 2
# gs_contribution: one record per Gaussian in caller order; sum in units of 2^-24
CONTRIBUTION_DTYPE = np.dtype([("sum", "<u8"), ("hits", "<u4"), ("wmax", "<f4")])


class Contributions:
    """Per-Gaussian contribution scores (gs_contribution): n 16-byte records in a device Buffer that
    Renderer.render(..., contributions=...) accumulates into.  Frames never clear it: clear() does."""

    def __init__(self, device, n, buffer=None):
        self.device = device
        self.n = int(n)
        self.buffer = buffer if buffer is not None else Buffer(device, size=max(self.n, 1) * CONTRIBUTION_DTYPE.itemsize)

    @staticmethod
    def new(device, stream, n):
        """n zeroed records"""
        c = Contributions(device, n)
        c.clear(stream)
        return c

    def __len__(self):
        return self.n

    def clear(self, stream):
        """gs_contributions_clear: zeroes the n records; only enqueues"""
        _check(_L.gs_contributions_clear(self.buffer._h, stream._h, self.n))

    def download(self, stream):
        """the n records as a CONTRIBUTION_DTYPE array; blocking"""
        return self.buffer.download(stream, np.uint8)[:self.n * CONTRIBUTION_DTYPE.itemsize].view(CONTRIBUTION_DTYPE)

    def select(self, stream, selection, kind, lo, hi, op=SEL_SET):
        """gs_select_contribution: selection = selection op {i : lo <= v_i <= hi}, v the CONTRIB_* value of record i
        (SUM: sum * 2^-24, HITS: hits, MAX: wmax, each as binary32); only enqueues"""
        if not isinstance(selection, Selection):
            raise TypeError("selection must be a Selection")
        if len(selection) != self.n:
            raise ValueError("the selection has %d bits, the contributions %d records" % (len(selection), self.n))
        _check(_L.gs_select_contribution(selection._h, stream._h, self.buffer._h, int(kind), float(lo), float(hi), select_op(op)))

    def release(self):
        self.buffer.release()


class Snapshot:
    """gs_snapshot: the records of one selection of a GaussiansBuffer on the device, with its own copy of the mask
    (DESIGN.md §3.9).  Made by GaussiansBuffer.snapshot, written back by GaussiansBuffer.restore."""

    def __init__(self, device, pod, _handle):
        self.device, self.pod, self._h = device, pod, _handle

    @property
    def len(self):
        """n of the buffer it was taken from"""
        return _L.gs_snapshot_len(self._h)

    @property
    def count(self):
        """records it holds"""
        return _L.gs_snapshot_count(self._h)

    @property
    def nbytes(self):
        """device memory it owns"""
        return _L.gs_snapshot_bytes(self._h)

    def selection(self, stream, sel, op=SEL_SET):
        """sel = sel op (the snapshot's mask) (gs_snapshot_selection); only enqueues"""
        if not isinstance(sel, Selection):
            raise TypeError("sel must be a Selection, not %s" % type(sel).__name__)
        op = select_op(op)
        _check(_L.gs_snapshot_selection(self._h, stream._h, sel._h, op))

    def destroy(self):
        if self._h:
            _L.gs_snapshot_destroy(self._h)
            self._h = None


def box_from_bounds(lo, hi):
    """world_to_box (12 numbers, column-major 3 x 4) of the axis-aligned box [lo, hi]"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    half, mid = 0.5 * (hi - lo), 0.5 * (hi + lo)
    b = np.zeros((4, 3))
    b[0, 0], b[1, 1], b[2, 2] = 1.0 / half
    b[3] = -mid / half
    return b.reshape(-1).astype(np.float32)


# gs_edit.flags
EDIT_TRANSFORM, EDIT_ROTATE_SH, EDIT_COLOR, EDIT_OPACITY = 1, 2, 4, 8


def sh_rotation_matrices(rot):
    """gs_sh_rotation_matrices: the SH band matrices (3 x 3, 5 x 5, 7 x 7, float32) of the rotation `rot` (xyzw), as the
    edit applies them: sh'_k = sum_j D[k][j] sh_j per channel and band."""
    q = (C.c_float * 4)(*[float(v) for v in rot])
    d1, d2, d3 = np.zeros((3, 3), np.float32), np.zeros((5, 5), np.float32), np.zeros((7, 7), np.float32)
    _check(_L.gs_sh_rotation_matrices(q, _ptr(d1), _ptr(d2), _ptr(d3)))
    return d1, d2, d3


def _color_matrix(m):
    """12 floats, column-major 3 x 4, from 12 numbers in that order or from a 3 x 4 array (rows = output channels)"""
    a = np.asarray(m, dtype=np.float64)
    if a.shape == (3, 4):
        a = a.T
    if a.size != 12 or a.ndim > 2 or (a.ndim == 2 and a.shape != (4, 3)):
        raise ValueError("a colour matrix takes 12 numbers (3 x 4, column-major) or a 3 x 4 array")
    return a.reshape(-1).astype(np.float32)


def _color_affine(linear, offset):
    m = np.zeros((3, 4))
    m[:, :3] = linear
    m[:, 3] = offset
    return _color_matrix(m)


def color_override(rgb):
    """every selected Gaussian gets the colour `rgb` (0..1); the linear part is 0, so the SH rest coefficients are
    flattened with it"""
    return _color_affine(np.zeros((3, 3)), np.asarray(rgb, np.float64).reshape(3))


def color_exposure(stops):
    """rgb' = 2^stops rgb"""
    return _color_affine(np.eye(3) * 2.0 ** float(stops), 0.0)


def color_contrast(contrast, pivot=0.5):
    """rgb' = (rgb - pivot) contrast + pivot"""
    k = float(contrast)
    return _color_affine(np.eye(3) * k, float(pivot) * (1.0 - k))


_LUMA = np.array([0.2126, 0.7152, 0.0722])      # Rec. 709


def color_saturation(saturation):
    """rgb' = luma + saturation (rgb - luma), Rec. 709 luma: 0 is grey, 1 the identity"""
    s = float(saturation)
    return _color_affine(s * np.eye(3) + (1.0 - s) * np.outer(np.ones(3), _LUMA), 0.0)


def color_hue(degrees):
    """the rotation of rgb about the grey axis (1, 1, 1) by `degrees`"""
    a = np.deg2rad(float(degrees))
    c, s = np.cos(a), np.sin(a)
    k = np.ones(3) / np.sqrt(3.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return _color_affine(c * np.eye(3) + s * K + (1.0 - c) * np.outer(k, k), 0.0)


def edit(transform=None, rotate_sh=True, color=None, opacity=None, pivot=None):
    """The gs_edit of GaussiansBuffer.edit.  transform: a ModelTransformPod (uniform positive scale)
    applied to position, rotation / covariance and scale, and — with rotate_sh — to the SH rest coefficients.  pivot: the
    point that the transform's rotation and scale leave in place (p' = s R (p - pivot) + pivot + pos); it is folded into
    transform.pos here, on the host.  color: 12 numbers (3 x 4, column-major: rgb' = C (rgb, 1)), a 3 x 4 array, or the
    result of a color_* helper.  opacity: (o0, o1) for a' = o0 a + o1, or one number o0.  Arguments left None are not
    touched by the edit; the library checks the values."""
    e = Edit()
    if pivot is not None and transform is None:
        raise ValueError("a pivot goes with a transform")
    if transform is not None:
        if not isinstance(transform, ModelTransformPod):
            raise TypeError("transform must be a ModelTransformPod (model_transform_pod())")
        e.flags |= EDIT_TRANSFORM | (EDIT_ROTATE_SH if rotate_sh else 0)
        e.transform = model_transform_pod(tuple(transform.pos), tuple(transform.rot), tuple(transform.scale))
        if pivot is not None:
            c = np.asarray(pivot, np.float64).reshape(3)
            x, y, z, w = [float(v) for v in transform.rot]
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
            sr = R * np.asarray(tuple(transform.scale), np.float64)[None, :]
            e.transform.pos[:] = [float(v) for v in np.asarray(tuple(transform.pos), np.float64) + c - sr @ c]
    if color is not None:
        e.flags |= EDIT_COLOR
        e.color[:] = [float(v) for v in _color_matrix(color)]
    if opacity is not None:
        o = np.atleast_1d(np.asarray(opacity, np.float64))
        if o.shape not in ((1,), (2,)):
            raise ValueError("opacity takes (o0, o1) or one number")
        e.flags |= EDIT_OPACITY
        e.opacity[:] = [float(o[0]), float(o[1]) if o.size == 2 else 0.0]
    return e


class Renderer:
    """One render context (scratch buffers + stats) on a device: gs_render_frame."""

    def __init__(self, device):
        h = C.c_void_p()
        _check(_L.gs_renderer_create(device._h, C.byref(h)))
        self._h, self.device = h, device

    def set_timing(self, enabled):
        _check(_L.gs_renderer_set_timing(self._h, int(bool(enabled))))

    def reset_stats(self):
        _check(_L.gs_renderer_reset_stats(self._h))

    def set_frame_flags_target(self, device_word_ptr):
        """gs_renderer_set_frame_flags_target: device word (or None) that receives every following
        frame's flags in stream order (FRAME_FLAG_*; 0 = rendered)."""
        _check(_L.gs_renderer_set_frame_flags_target(self._h, C.c_void_p(device_word_ptr or 0)))

    def stats(self):
        st = FrameStats()
        _check(_L.gs_renderer_stats(self._h, C.byref(st)))
        return st

    def sort_info(self):
        """gs_renderer_sort_info: how the last frame sorted (MSD-first or LSD passes, largest bucket)."""
        si = SortInfo()
        _check(_L.gs_renderer_sort_info(self._h, C.byref(si)))
        return si

    def set_sort_mode(self, depth_msd=-1, tile_msd=-1):
        """gs_renderer_set_sort_mode: 1 MSD-first, 0 LSD passes, -1 the renderer chooses (default)."""
        _check(_L.gs_renderer_set_sort_mode(self._h, int(depth_msd), int(tile_msd)))

    def set_tile_masks(self, mode=-1):
        """gs_renderer_set_tile_masks: 1 / 0 pin tile rect version 4 / 3, -1 the renderer chooses (by scene size)."""
        _check(_L.gs_renderer_set_tile_masks(self._h, int(mode)))

    def set_rounds(self, mode=-1, first_round=0):
        """gs_renderer_set_rounds: 1 two-round frames (the nearest `first_round` visible Gaussians first, the rest without
        what lies in finished tiles), 0 one round, -1 the renderer chooses."""
        _check(_L.gs_renderer_set_rounds(self._h, int(mode), int(first_round)))

    def render(self, stream, gaussians, gaussian_transform, model_transform, camera,
               rgba_device_ptr, band=None, check=True, depth_device_ptr=None, pick_device_ptr=None,
               pick_threshold=0.5, hide=None, tint=None, tint_rgba=None, contributions=None):
        """gs_render_frame.  check=True (the validated use: tests, one-off renders) waits for the
        frame and, if it exceeded the pair capacity sized from earlier frames, renders it again
        with the grown buffers; check=False only enqueues (the pipelined use: a viewer's frame
        loop, bench.py) — call wait_frame() / synchronise the stream before reading the image.
        depth_device_ptr / pick_device_ptr: H x W f32 / u32 device planes that the same frame fills
        (gs_render_frame_aux): the depth sum (expected depth = depth / alpha) and the
        caller's index of the Gaussian that takes the pixel's alpha to pick_threshold (PICK_NONE).
        hide / tint: Selections of the buffer's length (gs_render_frame_sel): the frame culls the
        Gaussians of `hide` and mixes tint_rgba = (r, g, b, a) into the colour of those of `tint`.
        contributions: a Contributions (or a Buffer of at least 16 n bytes) that the frame's blend ACCUMULATES the
        per-Gaussian scores into (gs_render_frame_contrib); one round, no aux planes."""
        b0, b1 = band if band is not None else (0, 0xFFFFFFFF)
        fs = frame_selection(hide, tint, tint_rgba)
        if contributions is not None and (depth_device_ptr is not None or pick_device_ptr is not None):
            raise ValueError("a contribution frame takes no depth / pick planes")
        cbuf = contributions.buffer if isinstance(contributions, Contributions) else contributions
        aux = None
        if depth_device_ptr is not None or pick_device_ptr is not None:
            aux = AuxTargets(C.c_void_p(depth_device_ptr or 0), C.c_void_p(pick_device_ptr or 0),
                             float(pick_threshold), 0)
        for attempt in range(4):
            if cbuf is not None:
                # (a frame skipped for pair capacity left the records untouched: the retry adds once)
                _check(_L.gs_render_frame_contrib(self._h, stream._h, gaussians._h, C.byref(gaussian_transform),
                                                  C.byref(model_transform), C.byref(camera), b0, b1,
                                                  C.c_void_p(rgba_device_ptr), C.byref(fs) if fs is not None else None,
                                                  cbuf._h))
            elif fs is not None:
                _check(_L.gs_render_frame_sel(self._h, stream._h, gaussians._h, C.byref(gaussian_transform),
                                              C.byref(model_transform), C.byref(camera), b0, b1,
                                              C.c_void_p(rgba_device_ptr), C.byref(aux) if aux is not None else None,
                                              C.byref(fs)))
            elif aux is None:
                _check(_L.gs_render_frame(self._h, stream._h, gaussians._h, C.byref(gaussian_transform),
                                          C.byref(model_transform), C.byref(camera), b0, b1,
                                          C.c_void_p(rgba_device_ptr)))
            else:
                _check(_L.gs_render_frame_aux(self._h, stream._h, gaussians._h, C.byref(gaussian_transform),
                                              C.byref(model_transform), C.byref(camera), b0, b1,
                                              C.c_void_p(rgba_device_ptr), C.byref(aux)))
            if not check:
                return None
            try:
                return self.wait_frame()
            except (PairCapacityError, RankOrderError):
                if attempt == 3:
                    raise

    def wait_frame(self):
        """blocks until the last frame has completed; raises PairCapacityError / PairOverflowError"""
        fr = FrameResult()
        _check(_L.gs_renderer_wait_frame(self._h, C.byref(fr)))
        return fr

    def select_visible(self, stream, selection, x0, y0, x1, y1, mask_device_ptr=None, op=SEL_SET):
        """gs_renderer_select_visible: selection = selection op {Gaussians the LAST FRAME kept whose mean lies in
        [x0, x1) x [y0, y1) and, with an H x W byte plane on the device, on a nonzero byte of it}.  Enqueued behind that
        frame; does not block."""
        if not isinstance(selection, Selection):
            raise TypeError("selection must be a Selection")
        _check(_L.gs_renderer_select_visible(self._h, stream._h, selection._h, float(x0), float(y0), float(x1), float(y1),
                                             C.c_void_p(mask_device_ptr or 0), select_op(op)))

    def download_projected(self, n):
        proj = np.zeros(n, dtype=PROJECTED_DTYPE)
        tiles = np.zeros(n, dtype=np.uint32)
        _check(_L.gs_renderer_download_projected(self._h, _ptr(proj), _ptr(tiles), n))
        return proj, tiles

    def _pairs(self, fn):
        d = C.c_uint64()
        _check(fn(self._h, None, None, 0, C.byref(d)))
        keys = np.zeros(max(d.value, 1), dtype=np.uint64)
        idx = np.zeros(max(d.value, 1), dtype=np.uint32)
        _check(fn(self._h, _ptr(keys), _ptr(idx), d.value, C.byref(d)))
        return keys[:d.value], idx[:d.value]

    def download_sorted(self):
        return self._pairs(_L.gs_renderer_download_sorted)

    def download_ranges(self, num_tiles):
        r = np.zeros((num_tiles, 2), dtype=np.uint32)
        _check(_L.gs_renderer_download_ranges(self._h, _ptr(r), num_tiles))
        return r

    def destroy(self):
        if self._h:
            _L.gs_renderer_destroy(self._h)
            self._h = None


class FrameRing:
    """Frames in flight: `frames` renderers, each on a stream of its own PRIORITY, take the frames in turn
    (what a viewer with double / triple buffering does).  A frame is a chain of dependent kernels — latency-bound
    in its sorts, VALU-bound in its blend — so the frames of different renderers overlap on the device, provided
    their streams sit on different hardware queues: HIP keeps separate queues per priority level, streams of one
    priority may share a queue (gs_stream_create_with_priority).  Every frame is the frame its renderer would
    have rendered alone; only the order in which the device works on them changes.  No reference item (the
    viewer owns the frame loop)."""

    def __init__(self, device, frames=3):
        least, greatest = device.stream_priority_range()
        cycle = [greatest, least, 0] if least != greatest else [0]
        self.priorities = [cycle[k % len(cycle)] for k in range(max(1, int(frames)))]
        self.streams = [device.create_stream(priority=p) for p in self.priorities]
        self.renderers = [Renderer(device) for _ in self.streams]
        self._next = 0

    def __len__(self):
        return len(self.renderers)

    def render(self, gaussians, gaussian_transform, model_transform, camera, rgba_device_ptr, band=None, check=False,
               depth_device_ptr=None, pick_device_ptr=None, pick_threshold=0.5, hide=None, tint=None, tint_rgba=None,
               contributions=None):
        """enqueues one frame on the next lane; returns the lane's index (its stream: `streams[lane]`).  The
        depth / pick planes as in Renderer.render: a lane writes them while later lanes run, so each lane needs its own.
        hide / tint / tint_rgba as in Renderer.render; the selections must have been filled on a stream the lane's stream is
        ordered behind (or be synchronised) before the frame is enqueued.  contributions as in Renderer.render: the lanes
        may share one buffer (the adds are atomic)."""
        lane = self._next % len(self.renderers)
        self._next += 1
        self.renderers[lane].render(self.streams[lane], gaussians, gaussian_transform, model_transform, camera,
                                    rgba_device_ptr, band=band, check=check, depth_device_ptr=depth_device_ptr,
                                    pick_device_ptr=pick_device_ptr, pick_threshold=pick_threshold, hide=hide, tint=tint,
                                    tint_rgba=tint_rgba, contributions=contributions)
        return lane

    def wait(self):
        """blocks until every lane's last frame has completed; their FrameResults (raises as wait_frame does)"""
        return [r.wait_frame() for r in self.renderers]

    def synchronize(self):
        for s in self.streams:
            s.synchronize()

    def close(self):
        for r in self.renderers:
            r.destroy()
        for s in self.streams:
            s.close()
        self.renderers, self.streams = [], []


COMPARE_SSIM = 1      # GS_COMPARE_SSIM


@dataclasses.dataclass
class ImageMetrics:
    """gs_image_metrics: the raw fields of gs_image_compare, channels r g b a (SSIM: r g b), and what a
    caller derives from them on the host."""
    pixels: int
    finite: int
    differing: int
    bit_differing: int
    sum_sq: np.ndarray        # float64[4]
    sum_abs: np.ndarray       # float64[4]
    max_abs: np.ndarray       # float32[4]
    max_abs_at: np.ndarray    # uint32[4]
    ssim_sum: np.ndarray      # float64[3]
    ssim_finite: np.ndarray   # uint64[3]
    raw: bytes = b""          # the 176 bytes of the record as the library wrote it

    @property
    def mse(self):
        """sum_sq / finite per channel (NaN without a finite pixel)"""
        with np.errstate(all="ignore"):
            return self.sum_sq / np.float64(self.finite)

    @property
    def mse_rgb(self):
        """the mean squared error over the three colour channels of the finite pixels"""
        with np.errstate(all="ignore"):
            return float(((self.sum_sq[0] + self.sum_sq[1]) + self.sum_sq[2]) / np.float64(3 * self.finite))

    def psnr(self, data_range=1.0):
        """10 log10(L^2 / mse_rgb); inf when the colour channels are equal"""
        m = self.mse_rgb
        if m == 0.0:
            return float("inf")
        return float(10.0 * np.log10(float(data_range) ** 2 / m))

    @property
    def ssim_channels(self):
        """ssim_sum / ssim_finite per colour channel (NaN without the SSIM flag)"""
        with np.errstate(all="ignore"):
            return self.ssim_sum / self.ssim_finite.astype(np.float64)

    @property
    def ssim(self):
        """the mean of the three channel means"""
        c = self.ssim_channels
        return float(((c[0] + c[1]) + c[2]) / 3.0)

    @property
    def identical(self):
        return self.bit_differing == 0


def _device_address(p, what):
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)):
        raise TypeError("%s must be a device address (an integer), not %s" % (what, type(p).__name__))
    return int(p)


def image_compare(device, stream, a_ptr, b_ptr, width, height, ssim=False, data_range=1.0, err_plane_ptr=None, ssim_plane_ptr=None):
    """gs_image_compare: an ImageMetrics of the two device images a, b (H x W x 4 float32 each, 16-byte
    aligned, e.g. Buffer.device_ptr() of two frames) — error sums, maxima and counts per channel and, with ssim=True, the
    sums of the 11 x 11-window SSIM of the colour channels.  err_plane_ptr / ssim_plane_ptr: device H x W float32 planes
    that receive the per-pixel largest |difference| / mean SSIM.  Blocking; stream None: the device's internal stream."""
    if not isinstance(device, Device):
        raise TypeError("device must be a Device, not %s" % type(device).__name__)
    if stream is not None and not isinstance(stream, Stream):
        raise TypeError("stream must be a Stream or None, not %s" % type(stream).__name__)
    a, b = _device_address(a_ptr, "a_ptr"), _device_address(b_ptr, "b_ptr")
    for name, v in (("width", width), ("height", height)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError("%s must be an integer, not %s" % (name, type(v).__name__))
    if not (0 < int(width) <= 0xFFFFFFFF and 0 < int(height) <= 0xFFFFFFFF) or int(width) * int(height) > 0xFFFFFFFE:
        raise ValueError("an image of %d x %d pixels cannot be compared" % (width, height))
    L = float(data_range)
    with np.errstate(over="ignore"):
        L32 = np.float32(L)
    if not (np.isfinite(L32) and L32 > 0):
        raise ValueError("data_range must be finite and positive, not %r" % (data_range,))
    if ssim_plane_ptr is not None and not ssim:
        raise ValueError("ssim_plane_ptr needs ssim=True")
    d = _capi.ImageCompareDesc()
    d.flags = COMPARE_SSIM if ssim else 0
    d.data_range = L
    d.err_plane = _device_address(err_plane_ptr, "err_plane_ptr") if err_plane_ptr is not None else None
    d.ssim_plane = _device_address(ssim_plane_ptr, "ssim_plane_ptr") if ssim_plane_ptr is not None else None
    out = _capi.ImageMetricsRecord()
    _check(_L.gs_image_compare(device._h, stream._h if stream is not None else None, C.c_void_p(a), C.c_void_p(b), int(width),
                               int(height), C.byref(d), C.byref(out)))
    return ImageMetrics(pixels=int(out.pixels), finite=int(out.finite), differing=int(out.differing),
                        bit_differing=int(out.bit_differing), sum_sq=np.array(out.sum_sq[:], np.float64),
                        sum_abs=np.array(out.sum_abs[:], np.float64), max_abs=np.array(out.max_abs[:], np.float32),
                        max_abs_at=np.array(out.max_abs_at[:], np.uint32), ssim_sum=np.array(out.ssim_sum[:], np.float64),
                        ssim_finite=np.array(out.ssim_finite[:], np.uint64), raw=bytes(out))


def sort_pairs_u64(device, stream, keys, values, end_bit=64):
    """Device radix sort of host arrays (stable LSD on key bits [0, end_bit)); returns copies."""
    k = np.ascontiguousarray(keys, dtype=np.uint64).copy()
    v = np.ascontiguousarray(values, dtype=np.uint32).copy()
    _check(_L.gs_sort_pairs_u64(device._h, stream._h if stream else None, _ptr(k), _ptr(v), len(k), end_bit))
    return k, v


def exclusive_scan_u32(device, stream, values):
    a = np.ascontiguousarray(values, dtype=np.uint32)
    out = np.zeros_like(a)
    total = C.c_uint64()
    _check(_L.gs_exclusive_scan_u32(device._h, stream._h if stream else None, _ptr(a), _ptr(out),
                                    len(a), C.byref(total)))
    return out, total.value
