// gs3d.hpp — header-only C++17 mirror of wgpu-3dgs-core's Rust API over the C ABI (gs3d.h).
//
// Rust is not available in the build image, so this is the compiled-language host mirror the
// reference's users would recognise: same type names, same methods, Result<_, E> -> exceptions
// carrying the variant fields of src/error.rs.  Citations are relative to the reference.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gs3d.h"

namespace gs3d {

// ---- errors (src/error.rs:55-143) --------------------------------------------------------------
struct Error : std::runtime_error {
    gs_status status;
    uint64_t a, b, c;
    Error(const gs_error_info &i) : std::runtime_error(i.message), status(i.code), a(i.a), b(i.b), c(i.c) {}
};
struct GaussiansBufferUpdateError : Error { using Error::Error; uint64_t count() const { return a; } uint64_t expected_count() const { return b; } };
struct GaussiansBufferUpdateRangeError : Error { using Error::Error; uint64_t count() const { return a; } uint64_t start() const { return b; } uint64_t expected_count() const { return c; } };
struct GaussiansBufferTryFromBufferError : Error { using Error::Error; uint64_t buffer_size() const { return a; } uint64_t expected_multiple_size() const { return b; } };
struct FixedSizeBufferWrapperError : Error { using Error::Error; uint64_t buffer_size() const { return a; } uint64_t expected_size() const { return b; } };
struct ComputeBundleCreateError : Error { using Error::Error; };
struct ComputeBundleBuildError : std::runtime_error { using std::runtime_error::runtime_error; };
struct DownloadBufferError : Error { using Error::Error; };
struct LossyConfigError : Error { using Error::Error; };   // where the reference panics
struct NoDeviceError : Error { using Error::Error; };
struct PlyError : Error { using Error::Error; };   // std::io::Error of the PLY reader
struct SpzError : Error { using Error::Error; };   // std::io::Error of the SPZ reader
// gs_renderer_wait_frame: the frame exceeded the pair capacity sized from earlier frames (render again)
struct PairCapacityError : Error { using Error::Error; uint64_t pairs() const { return a; } uint64_t capacity() const { return b; } };
struct RankOrderError : Error { using Error::Error; };   // the radix rank watchdog fired: render again

inline void check(gs_status s) {
    if (s == GS_OK) return;
    gs_error_info i;
    gs_last_error(&i);
    if (i.code != s) { i.code = s; std::strncpy(i.message, gs_status_string(s), sizeof(i.message) - 1); }
    switch (s) {
    case GS_ERR_COUNT_MISMATCH: throw GaussiansBufferUpdateError(i);
    case GS_ERR_RANGE_COUNT_MISMATCH: throw GaussiansBufferUpdateRangeError(i);
    case GS_ERR_BUFFER_SIZE_NOT_MULTIPLE: throw GaussiansBufferTryFromBufferError(i);
    case GS_ERR_BUFFER_SIZE_MISMATCHED: throw FixedSizeBufferWrapperError(i);
    case GS_ERR_RESOURCE_COUNT_MISMATCH:
    case GS_ERR_WORKGROUP_SIZE_EXCEEDS_LIMIT: throw ComputeBundleCreateError(i);
    case GS_ERR_DOWNLOAD: throw DownloadBufferError(i);
    case GS_ERR_LOSSY_CONFIG: throw LossyConfigError(i);
    case GS_ERR_NO_DEVICE: throw NoDeviceError(i);
    case GS_ERR_PLY: throw PlyError(i);
    case GS_ERR_SPZ: throw SpzError(i);
    case GS_ERR_PAIR_CAPACITY: throw PairCapacityError(i);
    case GS_ERR_RANK_ORDER: throw RankOrderError(i);
    default: throw Error(i);
    }
}

using Gaussian = gs_gaussian;   // src/gaussian.rs:53-60

// ---- GaussianPod family (src/buffer/gaussian.rs:239-384) ---------------------------------------
template <gs_sh_config SH, gs_cov3d_config COV>
struct GaussianPod {
    static constexpr gs_sh_config sh = SH;
    static constexpr gs_cov3d_config cov3d = COV;
    static size_t size() { return gs_pod_size(SH, COV); }
    static std::vector<std::pair<std::string, bool>> features() {
        uint8_t f[7];
        check(gs_pod_features(SH, COV, f));
        std::vector<std::pair<std::string, bool>> out;
        for (uint32_t i = 0; i < 7; i++) out.emplace_back(gs_feature_name(i), f[i] != 0);
        return out;
    }
    // G::from_gaussian over a slice -> packed bytes
    static std::vector<uint8_t> from_gaussians(const std::vector<Gaussian> &g) {
        std::vector<uint8_t> pods(g.size() * size());
        check(gs_pack(SH, COV, g.data(), g.size(), pods.data()));
        return pods;
    }
    static std::vector<Gaussian> into_gaussians(const std::vector<uint8_t> &pods) {
        std::vector<Gaussian> g(pods.size() / size());
        check(gs_unpack_to_gaussian(SH, COV, pods.data(), g.size(), g.data()));
        return g;
    }
    // packed records of this layout -> packed records of layout (TO, rotation + scale), the covariance of a covariance layout
    // decomposed on the host (gs3d.h gs_decompose_pods; no reference item)
    template <gs_sh_config TO = SH>
    static std::vector<uint8_t> decompose(const std::vector<uint8_t> &pods) {
        const size_t n = pods.size() / size();
        std::vector<uint8_t> out(n * gs_pod_size(TO, GS_COV3D_ROT_SCALE));
        if (n) check(gs_decompose_pods(SH, COV, TO, pods.data(), n, out.data()));
        return out;
    }
};
// one covariance (xx, yx, zx, yy, zy, zz) -> unit quaternion xyzw, w >= 0, and three scales (gs3d.h gs_cov3d_decompose)
inline void cov3d_decompose(const float cov[6], float rot_xyzw[4], float scale[3]) { gs_cov3d_decompose(cov, rot_xyzw, scale); }
#define GS3D_POD(S, C, NAME) using NAME = GaussianPod<S, C>;
GS3D_POD(GS_SH_SINGLE, GS_COV3D_ROT_SCALE, GaussianPodWithShSingleCov3dRotScaleConfigs)
GS3D_POD(GS_SH_SINGLE, GS_COV3D_SINGLE, GaussianPodWithShSingleCov3dSingleConfigs)
GS3D_POD(GS_SH_SINGLE, GS_COV3D_HALF, GaussianPodWithShSingleCov3dHalfConfigs)
GS3D_POD(GS_SH_HALF, GS_COV3D_ROT_SCALE, GaussianPodWithShHalfCov3dRotScaleConfigs)
GS3D_POD(GS_SH_HALF, GS_COV3D_SINGLE, GaussianPodWithShHalfCov3dSingleConfigs)
GS3D_POD(GS_SH_HALF, GS_COV3D_HALF, GaussianPodWithShHalfCov3dHalfConfigs)
GS3D_POD(GS_SH_NORM8, GS_COV3D_ROT_SCALE, GaussianPodWithShNorm8Cov3dRotScaleConfigs)
GS3D_POD(GS_SH_NORM8, GS_COV3D_SINGLE, GaussianPodWithShNorm8Cov3dSingleConfigs)
GS3D_POD(GS_SH_NORM8, GS_COV3D_HALF, GaussianPodWithShNorm8Cov3dHalfConfigs)
GS3D_POD(GS_SH_NONE, GS_COV3D_ROT_SCALE, GaussianPodWithShNoneCov3dRotScaleConfigs)
GS3D_POD(GS_SH_NONE, GS_COV3D_SINGLE, GaussianPodWithShNoneCov3dSingleConfigs)
GS3D_POD(GS_SH_NONE, GS_COV3D_HALF, GaussianPodWithShNoneCov3dHalfConfigs)
#undef GS3D_POD

// ---- source formats (src/source_format/{ply,spz}.rs) --------------------------------------------
using PlyGaussianPod = gs_ply_gaussian_pod;   // ply.rs:11-21

class PlyGaussians {   // ply.rs:204-431 (both the Inria and Custom variants decode to pods here)
public:
    std::vector<PlyGaussianPod> pods;
    bool inria = true;
    static PlyGaussians read_from(const void *bytes, size_t len) {
        PlyGaussians p;
        size_t n = 0;
        int32_t is_inria = 0;
        check(gs_ply_read(bytes, len, nullptr, 0, &n, &is_inria));
        p.pods.resize(n);
        check(gs_ply_read(bytes, len, p.pods.data(), n, &n, &is_inria));
        p.inria = is_inria != 0;
        return p;
    }
    static PlyGaussians from_gaussians(const std::vector<Gaussian> &g) {   // FromIterator<Gaussian>
        PlyGaussians p;
        p.pods.resize(g.size());
        gs_gaussian_to_ply(g.data(), g.size(), p.pods.data());
        return p;
    }
    std::vector<uint8_t> write_to() const {
        size_t n = 0;
        check(gs_ply_write(pods.data(), pods.size(), nullptr, 0, &n));
        std::vector<uint8_t> out(n);
        check(gs_ply_write(pods.data(), pods.size(), out.data(), out.size(), &n));
        return out;
    }
    std::vector<Gaussian> iter_gaussian() const {   // IterGaussian
        std::vector<Gaussian> g(pods.size());
        gs_gaussian_from_ply(pods.data(), pods.size(), g.data());
        return g;
    }
    size_t len() const { return pods.size(); }
    bool is_empty() const { return pods.empty(); }
};

struct SpzGaussiansFromGaussianSliceOptions : gs_spz_options {   // spz.rs:962-999
    SpzGaussiansFromGaussianSliceOptions() { gs_spz_options_default(this); }
};

class SpzGaussians {   // spz.rs:514-959: keeps the decompressed payload (header + columns) as read / encoded
public:
    gs_spz_header header{};
    std::vector<uint8_t> payload;       // what write_decompressed emits: reading then writing keeps the columns
    std::vector<Gaussian> gaussians;    // Gaussian::from_spz of every point (what iter_gaussian yields)

    explicit SpzGaussians(std::vector<uint8_t> decompressed) : payload(std::move(decompressed)) {
        size_t n = 0;
        check(gs_spz_decode_decompressed(payload.data(), payload.size(), &header, nullptr, 0, &n));
        gaussians.resize(n);
        check(gs_spz_decode_decompressed(payload.data(), payload.size(), &header, gaussians.data(), n, &n));
    }
    static SpzGaussians read_from(const void *bytes, size_t len) { return SpzGaussians(sized(gs_spz_decompress, bytes, len)); }
    static SpzGaussians read_decompressed(const void *bytes, size_t len) {
        return SpzGaussians(std::vector<uint8_t>((const uint8_t *)bytes, (const uint8_t *)bytes + len));
    }
    static SpzGaussians from_gaussians_with_options(const std::vector<Gaussian> &g, const gs_spz_options &o = SpzGaussiansFromGaussianSliceOptions()) {
        return SpzGaussians(write_gaussians_decompressed(g, o));
    }
    static SpzGaussians from_gaussians(const std::vector<Gaussian> &g) { return from_gaussians_with_options(g); }
    std::vector<uint8_t> write_to() const { return sized(gs_spz_compress, payload.data(), payload.size()); }
    const std::vector<uint8_t> &write_decompressed() const { return payload; }
    // one-shot helpers over the fused entry points
    static std::vector<uint8_t> write_gaussians(const std::vector<Gaussian> &g, const gs_spz_options &o = SpzGaussiansFromGaussianSliceOptions()) { return sized(gs_spz_encode, g.data(), g.size(), &o); }
    static std::vector<uint8_t> write_gaussians_decompressed(const std::vector<Gaussian> &g, const gs_spz_options &o = SpzGaussiansFromGaussianSliceOptions()) { return sized(gs_spz_encode_decompressed, g.data(), g.size(), &o); }
    const std::vector<Gaussian> &iter_gaussian() const { return gaussians; }
    size_t len() const { return gaussians.size(); }
    bool is_empty() const { return gaussians.empty(); }
    bool operator==(const SpzGaussians &o) const { return payload == o.payload; }

private:
    template <class F, class... A>
    static std::vector<uint8_t> sized(F fn, A... head) {   // the ABI's two-call pattern: size query, then fill
        size_t n = 0;
        check(fn(head..., nullptr, 0, &n));
        std::vector<uint8_t> out(n);
        check(fn(head..., out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }
};

// Gaussians / GaussiansSource (src/gaussian.rs:394-548): the format-agnostic read / write over the
// fused entry points gs_gaussians_read / gs_gaussians_write.  Source::Internal cannot be read from or
// written to a byte buffer (the reference's io::Error messages come back in Error::what()).
enum class GaussiansSource : uint32_t { Internal = GS_SOURCE_INTERNAL, Ply = GS_SOURCE_PLY, Spz = GS_SOURCE_SPZ };

class Gaussians {
public:
    GaussiansSource source = GaussiansSource::Internal;
    std::vector<Gaussian> gaussians;

    static Gaussians from_gaussians(std::vector<Gaussian> g) {
        Gaussians out;
        out.gaussians = std::move(g);
        return out;
    }
    static Gaussians read_from(const void *bytes, size_t len, GaussiansSource source) {
        Gaussians out;
        out.source = source;
        size_t n = 0;
        check(gs_gaussians_read(bytes, len, (gs_gaussians_source)source, nullptr, 0, &n));
        out.gaussians.resize(n);
        check(gs_gaussians_read(bytes, len, (gs_gaussians_source)source, out.gaussians.data(), n, &n));
        return out;
    }
    // write in `as` (default: the format the Gaussians were read from)
    std::vector<uint8_t> write_to(GaussiansSource as) const {
        size_t n = 0;
        check(gs_gaussians_write(gaussians.data(), gaussians.size(), (gs_gaussians_source)as, nullptr, 0, &n));
        std::vector<uint8_t> out(n);
        check(gs_gaussians_write(gaussians.data(), gaussians.size(), (gs_gaussians_source)as, out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }
    std::vector<uint8_t> write_to() const { return write_to(source); }
    const std::vector<Gaussian> &iter_gaussian() const { return gaussians; }
    size_t len() const { return gaussians.size(); }
    bool is_empty() const { return gaussians.empty(); }
};

// ---- device / stream / buffer --------------------------------------------------------------------
class Device {
  public:
    explicit Device(int ordinal = 0) { check(gs_device_create(ordinal, &h_)); }
    ~Device() { gs_device_destroy(h_); }
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
    gs_limits limits() const { gs_limits l; check(gs_device_limits(h_, &l)); return l; }
    bool fast_rank() const { return gs_device_fast_rank(h_) != 0; }
    gs_device *raw() const { return h_; }
  private:
    gs_device *h_ = nullptr;
};

class Stream {   // CommandEncoder + queue.submit
  public:
    explicit Stream(Device &d) { check(gs_stream_create(d.raw(), &h_)); }
    Stream(Device &d, int priority) { check(gs_stream_create_with_priority(d.raw(), priority, &h_)); }   // frames in flight: one priority each
    ~Stream() { gs_stream_destroy(h_); }
    Stream(const Stream &) = delete;
    void synchronize() { check(gs_stream_synchronize(h_)); }
    gs_stream *raw() const { return h_; }
  private:
    gs_stream *h_ = nullptr;
};

class Buffer {   // wgpu::Buffer + BufferWrapper (src/buffer/mod.rs:17-102); Clone = handle copy
  public:
    Buffer(Device &d, size_t bytes, const void *init = nullptr) { check(gs_buffer_create(d.raw(), bytes, init, &h_)); }
    explicit Buffer(gs_buffer *retained) : h_(retained) {}
    Buffer(const Buffer &o) : h_(gs_buffer_retain(o.h_)) {}
    Buffer(Buffer &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Buffer &operator=(Buffer o) { std::swap(h_, o.h_); return *this; }
    ~Buffer() { gs_buffer_release(h_); }
    size_t size() const { return gs_buffer_size(h_); }
    void *device_ptr() const { return gs_buffer_device_ptr(h_); }
    void write(Stream &s, size_t offset, const void *src, size_t bytes) { check(gs_buffer_write(h_, s.raw(), offset, src, bytes)); }
    template <class T> std::vector<T> download(Stream &s) const {   // BufferWrapper::download::<T>
        std::vector<T> out(size() / sizeof(T));
        check(gs_buffer_download(h_, s.raw(), out.data(), out.size() * sizeof(T)));
        return out;
    }
    // BufferWrapper::prepare_download / map_download (src/buffer/mod.rs:48-101): the copy is
    // enqueued now and mapped (waited for) later
    class Download {
      public:
        explicit Download(gs_download *d) : d_(d) {}
        Download(Download &&o) noexcept : d_(o.d_) { o.d_ = nullptr; }
        Download(const Download &) = delete;
        ~Download() { gs_download_release(d_); }
        bool ready() const { return gs_download_ready(d_) != 0; }
        template <class T> std::vector<T> map() {
            const void *p = nullptr;
            size_t n = 0;
            check(gs_download_map(d_, &p, &n));
            const T *t = static_cast<const T *>(p);
            return std::vector<T>(t, t + n / sizeof(T));
        }
      private:
        gs_download *d_;
    };
    Download prepare_download(Stream &s) const { gs_download *d = nullptr; check(gs_buffer_prepare_download(h_, s.raw(), &d)); return Download(d); }
    // the bytes [offset, offset + len) as a Huffman-only gzip member deflated on the device (gs3d.h gs_buffer_gzip_fast,
    // DESIGN.md 3.15; no reference item): byte-equal to gs3d::gzip_fast of the same bytes; blocking
    std::vector<uint8_t> gzip_fast(Stream &s, size_t offset, size_t len) const;
    gs_buffer *raw() const { return h_; }
  private:
    gs_buffer *h_ = nullptr;
};

class Selection;

// ---- snapshots (gs3d.h gs_snapshot; no reference item) --------------------------------
// The records of one selection of a buffer on the device, with its own copy of the mask: made by
// GaussiansBuffer::snapshot, written back by GaussiansBuffer::restore.  Move-only; the destructor synchronises the device.
class Snapshot {
  public:
    explicit Snapshot(gs_snapshot *h) : h_(h) {}
    Snapshot(Snapshot &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Snapshot &operator=(Snapshot &&o) noexcept { std::swap(h_, o.h_); return *this; }
    Snapshot(const Snapshot &) = delete;
    Snapshot &operator=(const Snapshot &) = delete;
    ~Snapshot() { gs_snapshot_destroy(h_); }
    size_t len() const { return gs_snapshot_len(h_); }          // n of the buffer it was taken from
    uint64_t count() const { return gs_snapshot_count(h_); }    // records it holds
    size_t bytes() const { return gs_snapshot_bytes(h_); }      // device memory it owns
    // sel = sel op (the snapshot's mask); only enqueues
    void selection(Stream &s, Selection &sel, gs_select_op op = GS_SEL_SET) const;
    gs_snapshot *raw() const { return h_; }
  private:
    gs_snapshot *h_ = nullptr;
};

// tag of the GaussiansBuffer::concat overload that converts its sources to the target layout: concat(s, converted, {...})
struct converted_t { explicit converted_t() = default; };
inline constexpr converted_t converted{};

template <class G>
class GaussiansBuffer {   // src/buffer/gaussian.rs:17-229
  public:
    GaussiansBuffer(Device &d, const std::vector<Gaussian> &g) { check(gs_gaussians_buffer_create_from_gaussians(d.raw(), G::sh, G::cov3d, g.data(), g.size(), &h_)); }
    // PlyGaussians -> buffer with Gaussian::from_ply + G::from_gaussian fused in one device kernel
    static GaussiansBuffer new_from_ply(Device &d, const std::vector<PlyGaussianPod> &ply) { GaussiansBuffer b; check(gs_gaussians_buffer_create_from_ply(d.raw(), G::sh, G::cov3d, ply.data(), ply.size(), &b.h_)); return b; }
    // SPZ file bytes -> buffer: host inflate, then Gaussian::from_spz + G::from_gaussian in one device kernel
    static GaussiansBuffer new_from_spz(Device &d, const void *bytes, size_t len) { GaussiansBuffer b; check(gs_gaussians_buffer_create_from_spz(d.raw(), G::sh, G::cov3d, bytes, len, nullptr, &b.h_)); return b; }
    void update_range_from_ply(Stream &s, size_t start, const std::vector<PlyGaussianPod> &ply) { check(gs_gaussians_buffer_update_range_ply(h_, s.raw(), start, ply.data(), ply.size())); }
    static GaussiansBuffer new_with_pods(Device &d, const std::vector<uint8_t> &pods) { GaussiansBuffer b; check(gs_gaussians_buffer_create(d.raw(), G::sh, G::cov3d, pods.data(), pods.size() / G::size(), &b.h_)); return b; }
    static GaussiansBuffer new_empty(Device &d, size_t len) { GaussiansBuffer b; check(gs_gaussians_buffer_create(d.raw(), G::sh, G::cov3d, nullptr, len, &b.h_)); return b; }
    static GaussiansBuffer try_from(const Buffer &buf) { GaussiansBuffer b; check(gs_gaussians_buffer_from_buffer(buf.raw(), G::sh, G::cov3d, &b.h_)); return b; }
    GaussiansBuffer(GaussiansBuffer &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    GaussiansBuffer(const GaussiansBuffer &) = delete;
    ~GaussiansBuffer() { gs_gaussians_buffer_destroy(h_); }
    size_t len() const { return gs_gaussians_buffer_len(h_); }
    bool is_empty() const { return len() == 0; }
    Buffer buffer() const { return Buffer(gs_buffer_retain(gs_gaussians_buffer_buffer(h_))); }
    void update(Stream &s, const std::vector<Gaussian> &g) { check(gs_gaussians_buffer_update_gaussians(h_, s.raw(), g.data(), g.size())); }
    void update_with_pod(Stream &s, const std::vector<uint8_t> &pods) { check(gs_gaussians_buffer_update(h_, s.raw(), pods.data(), pods.size() / G::size())); }
    void update_range(Stream &s, size_t start, const std::vector<Gaussian> &g) { check(gs_gaussians_buffer_update_range_gaussians(h_, s.raw(), start, g.data(), g.size())); }
    void update_range_with_pod(Stream &s, size_t start, const std::vector<uint8_t> &pods) { check(gs_gaussians_buffer_update_range(h_, s.raw(), start, pods.data(), pods.size() / G::size())); }
    std::vector<uint8_t> download(Stream &s) const { std::vector<uint8_t> out(len() * G::size()); check(gs_gaussians_buffer_download(h_, s.raw(), out.data(), len())); return out; }
    std::vector<Gaussian> download_gaussians(Stream &s) const { std::vector<Gaussian> out(len()); check(gs_gaussians_buffer_download_gaussians(h_, s.raw(), out.data(), len())); return out; }
    // renderer-side mirror order (gs3d.h: spatial by default); order[slot] = Gaussian index
    void set_spatial_order(bool enabled) { check(gs_gaussians_buffer_set_spatial_order(h_, enabled ? 1 : 0)); }
    bool spatial_order() const { return gs_gaussians_buffer_spatial_order(h_) != 0; }
    std::vector<uint32_t> download_order(Stream &s) const { std::vector<uint32_t> out(len()); check(gs_gaussians_buffer_download_order(h_, s.raw(), out.data(), out.size())); return out; }
    void mark_dirty() { gs_gaussians_buffer_mark_dirty(h_); }
    // edits of the selected Gaussians on the device (gs3d.h gs_gaussians_buffer_edit; no reference item):
    // sel == nullptr means every Gaussian; only enqueues on the stream
    void edit(Stream &s, const Selection *sel, const gs_edit &e);
    // a new buffer with the records of sel (invert: of its complement), caller order kept; blocking
    GaussiansBuffer extract(Stream &s, const Selection *sel, bool invert = false) const;
    // snapshots and concatenation (gs3d.h; no reference item).  snapshot: the records of sel (nullptr: all),
    // blocking.  restore: writes them back, only enqueues; exchange swaps instead (undo, then redo with the same snapshot).
    Snapshot snapshot(Stream &s, const Selection *sel = nullptr);
    void restore(Stream &s, Snapshot &snap, bool exchange = false) { check(gs_gaussians_buffer_restore(h_, s.raw(), snap.raw(), exchange ? 1 : 0)); }
    // a new buffer with the records of sels[i] of srcs[i] (sels empty, or a nullptr entry: all of that source), one source
    // after the other; counts (optional) receives the records taken per source.  Blocks once, for the counts.
    static GaussiansBuffer concat(Stream &s, const std::vector<const GaussiansBuffer *> &srcs, const std::vector<const Selection *> &sels = {},
                                  std::vector<uint64_t> *counts = nullptr);
    // layout conversion (gs3d.h gs_gaussians_buffer_create_converted / _create_concat_as; no reference item).
    // convert<To>: a new buffer of layout To with the converted records of sel (nullptr: all; invert: of its complement),
    // caller order kept; blocking.  concat(s, converted, ...): concat, but the sources may have any layouts (they are given
    // as raw handles, b.raw(), since their types differ) and each is converted to G, the target layout.  LossyConfigError
    // where a covariance would have to become rotation and scale (gs_layout_convertible).
    template <class To>
    GaussiansBuffer<To> convert(Stream &s, const Selection *sel = nullptr, bool invert = false) const;
    static GaussiansBuffer concat(Stream &s, converted_t, const std::vector<gs_gaussians_buffer *> &srcs,
                                  const std::vector<const Selection *> &sels = {}, std::vector<uint64_t> *counts = nullptr);
    // decompose<SH>: a new buffer of layout (SH, rotation + scale) with the decomposed records of sel (nullptr: all; invert:
    // of its complement), caller order kept; blocking (gs3d.h gs_gaussians_buffer_create_decomposed; no
    // reference item).  The covariance of a covariance layout becomes a unit quaternion and three scales, which the exports
    // and a rotation + scale scene accept; a rotation + scale source is convert.
    template <gs_sh_config SH = G::sh>
    GaussiansBuffer<GaussianPod<SH, GS_COV3D_ROT_SCALE>> decompose(Stream &s, const Selection *sel = nullptr, bool invert = false) const;
    // attribute statistics and histograms over the records of sel (nullptr: all) in one pass on the device (gs3d.h
    // gs_gaussians_buffer_stats / _histogram; no reference item); blocking.  mt == nullptr: the default
    // transform; ref == nullptr: the origin.  histogram: 2 x (bins + 3) counts, row 0 = the selection, row 1 = the others.
    gs_stats stats(Stream &s, const Selection *sel = nullptr, const gs_model_transform_pod *mt = nullptr, const float *ref = nullptr) const;
    std::vector<uint64_t> histogram(Stream &s, const gs_attribute_desc &a, float lo, float hi, uint32_t bins, const Selection *sel = nullptr) const;
    // counts[i] = min(c_i, cap), one uint32_t per Gaussian: the Gaussians of among (nullptr: all) with a finite world position
    // within radius of Gaussian i (gs3d.h gs_gaussians_buffer_neighbor_counts; no reference item); only
    // enqueues.  counts holds at least 4 len() bytes; read it back with Buffer::download.
    void neighbor_counts(Stream &s, float radius, uint32_t cap, Buffer &counts, const Selection *among = nullptr,
                         const gs_model_transform_pod *mt = nullptr);
    // the connected components of the neighbour graph within radius (gs3d.h gs_gaussians_buffer_components, DESIGN.md 3.16;
    // no reference item); only enqueues.  labels[i] = the smallest index of i's component (GS_COMPONENT_NONE: no point),
    // sizes[i] = its number of points (0: no point), 4 len() bytes each; info = one gs_components_info.  Each may be nullptr,
    // not all three.
    void components(Stream &s, float radius, Buffer *labels, Buffer *sizes, Buffer *info, const Selection *among = nullptr,
                    const gs_model_transform_pod *mt = nullptr);
    // simplify<To>: a new buffer of layout To (default: this one's; every layout is a valid target) in which the Gaussians
    // of among (nullptr: all) that share a grid cell of side cell_size are merged into one, in cell order; blocking (gs3d.h
    // gs_gaussians_buffer_create_simplified; no reference item).  cell_of (nullptr, or at least 4 len()
    // bytes): word i = the record of the result Gaussian i went into, 0xffffffff where it is no point.
    template <class To = G>
    GaussiansBuffer<To> simplify(Stream &s, float cell_size, const Selection *among = nullptr, Buffer *cell_of = nullptr) const;
    // the k nearest other Gaussians of among (nullptr: all) within radius of every Gaussian of queries (nullptr: all): row i
    // of dist2 = k binary32 squared distances ascending, padded with +inf; row i of index (nullptr: not wanted) = their
    // indices, padded with GS_KNN_NONE; NaN rows where i is no point (gs3d.h gs_gaussians_buffer_knn; no
    // reference item); only enqueues.  A plane holds at least 4 k len() bytes; rows outside queries keep their bytes.
    void knn(Stream &s, uint32_t k, float radius, Buffer &dist2, Buffer *index = nullptr, const Selection *among = nullptr,
             const Selection *queries = nullptr, const gs_model_transform_pod *mt = nullptr);
    // the k nearest Gaussians of ANOTHER buffer (among: a selection of target, nullptr: all) within radius of every Gaussian of
    // queries (nullptr: all) of this one, each side under its own transform: the planes of knn, row i in this buffer's order,
    // index holding target indices (gs3d.h gs_gaussians_buffer_knn_between; no reference item); only enqueues.
    template <class T>
    void knn_to(Stream &s, GaussiansBuffer<T> &target, uint32_t k, float radius, Buffer &dist2, Buffer *index = nullptr,
                const Selection *queries = nullptr, const Selection *among = nullptr, const gs_model_transform_pod *mt = nullptr,
                const gs_model_transform_pod *target_mt = nullptr);
    // the sums over the pairs (Gaussian i of queries, Gaussian index[i k] of target) that gs_rigid_fit reads; an index at or
    // beyond target.len() names no pair (gs3d.h gs_gaussians_buffer_pair_sums; no reference item); blocking.
    template <class T>
    gs_pair_sums pair_sums(Stream &s, GaussiansBuffer<T> &target, const Buffer &index, uint32_t k = 1, const Selection *queries = nullptr,
                           const gs_model_transform_pod *mt = nullptr, const gs_model_transform_pod *target_mt = nullptr);
    // the .spz file image of the records of sel (nullptr: all; invert: of its complement), the payload deflated on the device
    // (gs3d.h gs_gaussians_buffer_export_spz_fast; no reference item); options == nullptr: the defaults.
    // Inflates to what gs_gaussians_buffer_export_spz_decompressed gives; blocking.
    std::vector<uint8_t> export_spz_fast(Stream &s, const Selection *sel = nullptr, bool invert = false, const gs_spz_options *options = nullptr) const;
    gs_gaussians_buffer *raw() const { return h_; }
  private:
    template <class> friend class GaussiansBuffer;      // convert<To> builds a buffer of another layout
    GaussiansBuffer() = default;
    gs_gaussians_buffer *h_ = nullptr;
};

// ---- selections (gs3d.h gs_selection; no reference item) ------------------------------
// One bit per Gaussian of a buffer, in the caller's index order, on the device.  Every call but download / count only
// enqueues on the stream.
class Selection {
  public:
    Selection(Device &d, size_t n) { check(gs_selection_create(d.raw(), n, &h_)); }
    Selection(Selection &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Selection(const Selection &) = delete;
    ~Selection() { gs_selection_destroy(h_); }
    size_t len() const { return gs_selection_len(h_); }
    size_t words() const { return (len() + 31) / 32; }
    void clear(Stream &s) { check(gs_selection_clear(h_, s.raw())); }
    void fill(Stream &s) { check(gs_selection_fill(h_, s.raw())); }
    void invert(Stream &s) { check(gs_selection_invert(h_, s.raw())); }
    void combine(Stream &s, gs_select_op op, const Selection &src) { check(gs_selection_combine(h_, s.raw(), op, src.h_)); }
    void upload(Stream &s, const std::vector<uint32_t> &w) { check(gs_selection_upload(h_, s.raw(), w.data(), w.size())); }
    std::vector<uint32_t> download(Stream &s) const { std::vector<uint32_t> w(words()); check(gs_selection_download(h_, s.raw(), w.data(), w.size())); return w; }
    uint64_t count(Stream &s) const { uint64_t c = 0; check(gs_selection_count(h_, s.raw(), &c)); return c; }
    template <class G>
    void select_sphere(Stream &s, GaussiansBuffer<G> &g, const gs_model_transform_pod &mt, const float center[3], float radius,
                       gs_select_op op = GS_SEL_SET) { check(gs_select_sphere(h_, s.raw(), g.raw(), &mt, center, radius, op)); }
    template <class G>
    void select_box(Stream &s, GaussiansBuffer<G> &g, const gs_model_transform_pod &mt, const float world_to_box[12],
                    gs_select_op op = GS_SEL_SET) { check(gs_select_box(h_, s.raw(), g.raw(), &mt, world_to_box, op)); }
    // sel = sel op {i : start <= i < start + count}; only enqueues
    void select_range(Stream &s, size_t start, size_t count, gs_select_op op = GS_SEL_SET) { check(gs_select_range(h_, s.raw(), start, count, op)); }
    // sel = sel op {i : lo <= attribute_i <= hi} (gs_select_attribute); only enqueues
    template <class G>
    void select_attribute(Stream &s, GaussiansBuffer<G> &g, const gs_attribute_desc &a, float lo, float hi,
                          gs_select_op op = GS_SEL_SET) { check(gs_select_attribute(h_, s.raw(), g.raw(), &a, lo, hi, op)); }
    // sel = sel op {i : min_count <= c_i <= max_count}, c_i as GaussiansBuffer::neighbor_counts without a cap
    // (gs_select_neighbors); only enqueues.  max_count = k - 1: the floaters with fewer than k others around
    template <class G>
    void select_neighbors(Stream &s, GaussiansBuffer<G> &g, float radius, uint32_t min_count = 0, uint32_t max_count = UINT32_MAX,
                          const Selection *among = nullptr, const gs_model_transform_pod *mt = nullptr, gs_select_op op = GS_SEL_SET) {
        check(gs_select_neighbors(h_, s.raw(), g.raw(), among ? among->raw() : nullptr, mt, radius, min_count, max_count, op));
    }
    // sel = sel op {i : min_size <= S_i <= max_size}, S_i the number of points in i's connected component within radius
    // (gs_select_components; no reference item); only enqueues.  max_size = m - 1: every cluster smaller than m
    template <class G>
    void select_components(Stream &s, GaussiansBuffer<G> &g, float radius, uint32_t min_size = 1, uint32_t max_size = UINT32_MAX,
                           const Selection *among = nullptr, const gs_model_transform_pod *mt = nullptr, gs_select_op op = GS_SEL_SET) {
        check(gs_select_components(h_, s.raw(), g.raw(), among ? among->raw() : nullptr, mt, radius, min_size, max_size, op));
    }
    // sel = sel op {i : i's connected component within radius holds a Gaussian of seeds} (gs_select_connected, DESIGN.md 3.16;
    // no reference item); only enqueues.  seeds may be *this: the selection grows to whole clusters
    template <class G>
    void select_connected(Stream &s, GaussiansBuffer<G> &g, float radius, const Selection &seeds, const Selection *among = nullptr,
                          const gs_model_transform_pod *mt = nullptr, gs_select_op op = GS_SEL_SET) {
        check(gs_select_connected(h_, s.raw(), g.raw(), among ? among->raw() : nullptr, mt, radius, seeds.raw(), op));
    }
    // sel = sel op {i : row i is a point's and lo <= v_i <= hi}, v the GS_KNN_* statistic of row i of the len() rows of k
    // values in dist2, a plane of GaussiansBuffer::knn (gs_select_knn; no reference item); only enqueues.
    // lo = hi = +inf: exactly the incomplete rows
    void select_knn(Stream &s, const Buffer &dist2, uint32_t k, uint32_t kind, float lo, float hi, gs_select_op op = GS_SEL_SET) {
        check(gs_select_knn(h_, s.raw(), dist2.raw(), k, kind, lo, hi, op));
    }
    // sel = sel op {i : lo <= v_i <= hi}, v the GS_CONTRIB_* value of record i of `contrib` (gs_select_contribution,
    // DESIGN.md 3.5c); only enqueues
    void select_contribution(Stream &s, Buffer &contrib, uint32_t kind, float lo, float hi, gs_select_op op = GS_SEL_SET) {
        check(gs_select_contribution(h_, s.raw(), contrib.raw(), kind, lo, hi, op));
    }
    gs_selection *raw() const { return h_; }
  private:
    gs_selection *h_ = nullptr;
};

// gs_contributions_clear: zeroes the n contribution records (16 n bytes) of `contrib`; only enqueues
inline void contributions_clear(Buffer &contrib, Stream &s, size_t n) { check(gs_contributions_clear(contrib.raw(), s.raw(), n)); }

inline void Snapshot::selection(Stream &s, Selection &sel, gs_select_op op) const { check(gs_snapshot_selection(h_, s.raw(), sel.raw(), op)); }
template <class G>
inline Snapshot GaussiansBuffer<G>::snapshot(Stream &s, const Selection *sel) {
    gs_snapshot *h = nullptr;
    check(gs_gaussians_buffer_snapshot(h_, s.raw(), sel ? sel->raw() : nullptr, &h));
    return Snapshot(h);
}
template <class G>
inline GaussiansBuffer<G> GaussiansBuffer<G>::concat(Stream &s, const std::vector<const GaussiansBuffer *> &srcs,
                                                     const std::vector<const Selection *> &sels, std::vector<uint64_t> *counts) {
    if (!sels.empty() && sels.size() != srcs.size()) throw std::invalid_argument("concat: one selection per source, or none");
    std::vector<gs_gaussians_buffer *> g;
    std::vector<const gs_selection *> m;
    for (auto *b : srcs) g.push_back(b ? b->raw() : nullptr);
    for (auto *x : sels) m.push_back(x ? x->raw() : nullptr);
    if (counts) counts->assign(srcs.size(), 0);
    GaussiansBuffer b;
    check(gs_gaussians_buffer_create_concat(s.raw(), g.data(), m.empty() ? nullptr : m.data(), (uint32_t)g.size(), &b.h_,
                                            counts ? counts->data() : nullptr));
    return b;
}

template <class G>
template <class To>
inline GaussiansBuffer<To> GaussiansBuffer<G>::convert(Stream &s, const Selection *sel, bool invert) const {
    GaussiansBuffer<To> b;
    check(gs_gaussians_buffer_create_converted(h_, s.raw(), sel ? sel->raw() : nullptr, invert ? 1 : 0, To::sh, To::cov3d, &b.h_, nullptr));
    return b;
}
template <class G>
template <gs_sh_config SH>
inline GaussiansBuffer<GaussianPod<SH, GS_COV3D_ROT_SCALE>> GaussiansBuffer<G>::decompose(Stream &s, const Selection *sel, bool invert) const {
    GaussiansBuffer<GaussianPod<SH, GS_COV3D_ROT_SCALE>> b;
    check(gs_gaussians_buffer_create_decomposed(h_, s.raw(), sel ? sel->raw() : nullptr, invert ? 1 : 0, SH, &b.h_, nullptr));
    return b;
}
template <class G>
inline GaussiansBuffer<G> GaussiansBuffer<G>::concat(Stream &s, converted_t, const std::vector<gs_gaussians_buffer *> &srcs,
                                                          const std::vector<const Selection *> &sels, std::vector<uint64_t> *counts) {
    if (!sels.empty() && sels.size() != srcs.size()) throw std::invalid_argument("concat: one selection per source, or none");
    std::vector<const gs_selection *> m;
    for (auto *x : sels) m.push_back(x ? x->raw() : nullptr);
    if (counts) counts->assign(srcs.size(), 0);
    GaussiansBuffer b;
    check(gs_gaussians_buffer_create_concat_as(s.raw(), srcs.data(), m.empty() ? nullptr : m.data(), (uint32_t)srcs.size(), G::sh, G::cov3d,
                                               &b.h_, counts ? counts->data() : nullptr));
    return b;
}

template <class G>
inline gs_stats GaussiansBuffer<G>::stats(Stream &s, const Selection *sel, const gs_model_transform_pod *mt, const float *ref) const {
    gs_stats out;
    check(gs_gaussians_buffer_stats(h_, s.raw(), sel ? sel->raw() : nullptr, mt, ref, &out));
    return out;
}
template <class G>
inline std::vector<uint64_t> GaussiansBuffer<G>::histogram(Stream &s, const gs_attribute_desc &a, float lo, float hi, uint32_t bins,
                                                           const Selection *sel) const {
    std::vector<uint64_t> counts(2 * ((size_t)bins + 3));
    check(gs_gaussians_buffer_histogram(h_, s.raw(), sel ? sel->raw() : nullptr, &a, lo, hi, bins, counts.data()));
    return counts;
}

template <class G>
inline void GaussiansBuffer<G>::neighbor_counts(Stream &s, float radius, uint32_t cap, Buffer &counts, const Selection *among,
                                                const gs_model_transform_pod *mt) {
    check(gs_gaussians_buffer_neighbor_counts(h_, s.raw(), among ? among->raw() : nullptr, mt, radius, cap, counts.raw()));
}
template <class G>
inline void GaussiansBuffer<G>::components(Stream &s, float radius, Buffer *labels, Buffer *sizes, Buffer *info, const Selection *among,
                                           const gs_model_transform_pod *mt) {
    check(gs_gaussians_buffer_components(h_, s.raw(), among ? among->raw() : nullptr, mt, radius, labels ? labels->raw() : nullptr,
                                         sizes ? sizes->raw() : nullptr, info ? info->raw() : nullptr));
}

template <class G>
template <class To>
inline GaussiansBuffer<To> GaussiansBuffer<G>::simplify(Stream &s, float cell_size, const Selection *among, Buffer *cell_of) const {
    GaussiansBuffer<To> b;
    check(gs_gaussians_buffer_create_simplified(h_, s.raw(), among ? among->raw() : nullptr, cell_size, To::sh, To::cov3d,
                                                cell_of ? cell_of->raw() : nullptr, &b.h_, nullptr));
    return b;
}

template <class G>
inline void GaussiansBuffer<G>::knn(Stream &s, uint32_t k, float radius, Buffer &dist2, Buffer *index, const Selection *among,
                                    const Selection *queries, const gs_model_transform_pod *mt) {
    check(gs_gaussians_buffer_knn(h_, s.raw(), among ? among->raw() : nullptr, queries ? queries->raw() : nullptr, mt, k, radius,
                                  dist2.raw(), index ? index->raw() : nullptr));
}
// the summary of the GS_KNN_* statistic over the n rows of k values in dist2 (gs3d.h gs_knn_summary; no
// reference item); blocking
inline gs_knn_summary_result knn_summary(Stream &s, const Buffer &dist2, uint64_t n, uint32_t k, uint32_t kind) {
    gs_knn_summary_result r;
    check(gs_knn_summary(s.raw(), dist2.raw(), n, k, kind, &r));
    return r;
}

template <class G>
template <class T>
inline void GaussiansBuffer<G>::knn_to(Stream &s, GaussiansBuffer<T> &target, uint32_t k, float radius, Buffer &dist2, Buffer *index,
                                       const Selection *queries, const Selection *among, const gs_model_transform_pod *mt,
                                       const gs_model_transform_pod *target_mt) {
    check(gs_gaussians_buffer_knn_between(h_, target.raw(), s.raw(), queries ? queries->raw() : nullptr, among ? among->raw() : nullptr, mt,
                                          target_mt, k, radius, dist2.raw(), index ? index->raw() : nullptr));
}
template <class G>
template <class T>
inline gs_pair_sums GaussiansBuffer<G>::pair_sums(Stream &s, GaussiansBuffer<T> &target, const Buffer &index, uint32_t k,
                                                  const Selection *queries, const gs_model_transform_pod *mt,
                                                  const gs_model_transform_pod *target_mt) {
    gs_pair_sums r;
    check(gs_gaussians_buffer_pair_sums(h_, target.raw(), s.raw(), queries ? queries->raw() : nullptr, mt, target_mt, index.raw(), k, &r));
    return r;
}
// the similarity transform that brings the p of the pairs onto their q, acting in world space after the query's transform;
// *rms (nullptr: not wanted) = the RMS distance of the pairs as they came in (gs3d.h gs_rigid_fit; no reference
// item); host only
inline gs_model_transform_pod rigid_fit(const gs_pair_sums &sums, bool with_scale = false, double *rms = nullptr) {
    gs_model_transform_pod d;
    check(gs_rigid_fit(&sums, with_scale ? 1 : 0, &d, rms));
    return d;
}
// the pod of delta o m for a delta of uniform scale (gs3d.h gs_model_transform_compose; no reference item)
inline gs_model_transform_pod compose(const gs_model_transform_pod &delta, const gs_model_transform_pod &m) {
    gs_model_transform_pod r;
    gs_model_transform_compose(&delta, &m, &r);
    return r;
}

template <class G>
inline void GaussiansBuffer<G>::edit(Stream &s, const Selection *sel, const gs_edit &e) {
    check(gs_gaussians_buffer_edit(h_, s.raw(), sel ? sel->raw() : nullptr, &e));
}
template <class G>
inline GaussiansBuffer<G> GaussiansBuffer<G>::extract(Stream &s, const Selection *sel, bool invert) const {
    GaussiansBuffer b;
    check(gs_gaussians_buffer_create_from_selection(h_, s.raw(), sel ? sel->raw() : nullptr, invert ? 1 : 0, &b.h_, nullptr));
    return b;
}
// the SH band matrices of a rotation (xyzw), row-major 3x3, 5x5, 7x7 (gs3d.h gs_sh_rotation_matrices; no reference item)
struct ShRotation { float d1[9], d2[25], d3[49]; };
inline ShRotation sh_rotation_matrices(const float rot_xyzw[4]) {
    ShRotation r;
    check(gs_sh_rotation_matrices(rot_xyzw, r.d1, r.d2, r.d3));
    return r;
}

// GaussianTransformPod helpers (src/buffer/gaussian_transform.rs)
inline std::optional<gs_gaussian_transform_pod> gaussian_transform_pod(float size, gs_display_mode mode, uint8_t sh_deg, bool no_sh0, float max_std_dev) {
    gs_gaussian_transform_pod p;
    if (gs_gaussian_transform_pod_new(size, mode, sh_deg, no_sh0, max_std_dev, &p) != GS_OK) return std::nullopt;
    return p;
}
struct GaussianTransformBuffer : Buffer {   // :104-163
    explicit GaussianTransformBuffer(Device &d) : Buffer(make(d)) {}
    void update_with_pod(Stream &s, const gs_gaussian_transform_pod &p) { check(gs_gaussian_transform_buffer_update(raw(), s.raw(), &p)); }
    static GaussianTransformBuffer try_from(const Buffer &b) { check(gs_gaussian_transform_buffer_from_buffer(b.raw())); return GaussianTransformBuffer(b); }
  private:
    explicit GaussianTransformBuffer(const Buffer &b) : Buffer(b) {}
    static gs_buffer *make(Device &d) { gs_buffer *b; check(gs_gaussian_transform_buffer_create(d.raw(), &b)); return b; }
};
struct ModelTransformBuffer : Buffer {      // src/buffer/model_transform.rs:10-58
    explicit ModelTransformBuffer(Device &d) : Buffer(make(d)) {}
    void update(Stream &s, const float pos[3], const float rot[4], const float scale[3]) { gs_model_transform_pod p; gs_model_transform_pod_new(pos, rot, scale, &p); check(gs_model_transform_buffer_update(raw(), s.raw(), &p)); }
    static ModelTransformBuffer try_from(const Buffer &b) { check(gs_model_transform_buffer_from_buffer(b.raw())); return ModelTransformBuffer(b); }
  private:
    explicit ModelTransformBuffer(const Buffer &b) : Buffer(b) {}
    static gs_buffer *make(Device &d) { gs_buffer *b; check(gs_model_transform_buffer_create(d.raw(), &b)); return b; }
};

// ---- ComputeBundle (src/compute_bundle.rs) -------------------------------------------------------
class ComputeBundle {
  public:
    ComputeBundle(gs_bundle *h, bool managed) : h_(h), managed_(managed) {}
    ComputeBundle(ComputeBundle &&o) noexcept : h_(o.h_), managed_(o.managed_) { o.h_ = nullptr; }
    ~ComputeBundle() { gs_bundle_destroy(h_); }
    uint32_t workgroup_size() const { return gs_bundle_workgroup_size(h_); }
    std::optional<std::string> label() const { const char *l = gs_bundle_label(h_); return l ? std::optional<std::string>(l) : std::nullopt; }
    void dispatch(Stream &s, uint32_t count) { check(gs_bundle_dispatch(h_, s.raw(), count)); }
    void dispatch(Stream &s, uint32_t count, const std::vector<std::vector<const Buffer *>> &groups) {
        std::vector<std::vector<gs_buffer *>> raw(groups.size());
        std::vector<gs_buffer *const *> ptrs;
        std::vector<uint32_t> counts;
        for (size_t i = 0; i < groups.size(); i++) {
            for (auto *b : groups[i]) raw[i].push_back(b->raw());
            ptrs.push_back(raw[i].data());
            counts.push_back((uint32_t)raw[i].size());
        }
        check(gs_bundle_dispatch_with_bind_groups(h_, s.raw(), count, ptrs.data(), counts.data(), (uint32_t)groups.size()));
    }
    uint32_t last_workgroup_count() const { return gs_bundle_last_workgroup_count(h_); }
  private:
    gs_bundle *h_;
    bool managed_;
};

class ComputeBundleBuilder {   // :364-593; required fields checked in the reference's order (:505-519)
  public:
    ComputeBundleBuilder &label(std::string l) { label_ = std::move(l); return *this; }
    ComputeBundleBuilder &bind_group_layout(uint32_t bindings) { layouts_.push_back(bindings); return *this; }
    ComputeBundleBuilder &resolver() { resolver_ = true; return *this; }   // the built-in kernel registry
    ComputeBundleBuilder &entry_point(std::string e) { entry_ = std::move(e); return *this; }
    ComputeBundleBuilder &main_shader(gs_kernel_id k) { kernel_ = k; return *this; }
    template <class G> ComputeBundleBuilder &features() { sh_ = G::sh; cov_ = G::cov3d; return *this; }
    ComputeBundleBuilder &workgroup_size(uint32_t w) { wg_ = w; return *this; }
    ComputeBundleBuilder &constant(std::string name, double v) { cnames_.push_back(std::move(name)); cvals_.push_back(v); return *this; }
    ComputeBundle build(Device &d, const std::vector<std::vector<const Buffer *>> &resources) {
        validate();
        gs_bundle_desc desc = make_desc();
        std::vector<std::vector<gs_buffer *>> raw(resources.size());
        std::vector<gs_buffer *const *> ptrs;
        std::vector<uint32_t> counts;
        for (size_t i = 0; i < resources.size(); i++) {
            for (auto *b : resources[i]) raw[i].push_back(b->raw());
            ptrs.push_back(raw[i].data());
            counts.push_back((uint32_t)raw[i].size());
        }
        gs_bundle *h;
        check(gs_bundle_create_with_bind_groups(d.raw(), &desc, ptrs.data(), counts.data(), (uint32_t)resources.size(), &h));
        return ComputeBundle(h, true);
    }
    ComputeBundle build_without_bind_groups(Device &d) {
        validate();
        gs_bundle_desc desc = make_desc();
        gs_bundle *h;
        check(gs_bundle_create(d.raw(), &desc, &h));
        return ComputeBundle(h, false);
    }
  private:
    void validate() const {
        if (layouts_.empty()) throw ComputeBundleBuildError("missing bind group layout for compute bundle");
        if (!resolver_) throw ComputeBundleBuildError("missing resolver for compute bundle");
        if (!entry_) throw ComputeBundleBuildError("missing entry point for compute bundle");
        if (!kernel_) throw ComputeBundleBuildError("missing main shader for compute bundle");
    }
    gs_bundle_desc make_desc() {
        cptrs_.clear();
        for (auto &n : cnames_) cptrs_.push_back(n.c_str());
        gs_bundle_desc d{};
        d.label = label_ ? label_->c_str() : nullptr;
        d.kernel = *kernel_;
        d.sh = sh_;
        d.cov = cov_;
        d.bind_group_count = (uint32_t)layouts_.size();
        d.bindings_per_group = layouts_.data();
        d.workgroup_size = wg_;
        d.constant_names = cptrs_.data();
        d.constant_values = cvals_.data();
        d.constant_count = (uint32_t)cvals_.size();
        return d;
    }
    std::optional<std::string> label_, entry_;
    std::vector<uint32_t> layouts_;
    bool resolver_ = false;
    std::optional<gs_kernel_id> kernel_;
    gs_sh_config sh_ = GS_SH_SINGLE;
    gs_cov3d_config cov_ = GS_COV3D_ROT_SCALE;
    uint32_t wg_ = 0;
    std::vector<std::string> cnames_;
    std::vector<const char *> cptrs_;
    std::vector<double> cvals_;
};

// ---- renderer ------------------------------------------------------------------------------------
class Renderer {
  public:
    explicit Renderer(Device &d) { check(gs_renderer_create(d.raw(), &h_)); }
    ~Renderer() { gs_renderer_destroy(h_); }
    Renderer(const Renderer &) = delete;
    template <class G>
    void render(Stream &s, GaussiansBuffer<G> &g, const gs_gaussian_transform_pod &gt, const gs_model_transform_pod &mt,
                const gs_camera &cam, float *rgba_device, uint32_t band_ty0 = 0, uint32_t band_ty1 = 0xffffffffu) {
        check(gs_render_frame(h_, s.raw(), g.raw(), &gt, &mt, &cam, band_ty0, band_ty1, rgba_device));
    }
    // the same frame with its depth / pick planes (gs_render_frame_aux; aux == nullptr: render() above).  The band is
    // spelled out (0, 0xffffffff: the whole image) so that no call of the overload above can mean this one.
    template <class G>
    void render(Stream &s, GaussiansBuffer<G> &g, const gs_gaussian_transform_pod &gt, const gs_model_transform_pod &mt,
                const gs_camera &cam, float *rgba_device, uint32_t band_ty0, uint32_t band_ty1, const gs_aux_targets *aux) {
        check(gs_render_frame_aux(h_, s.raw(), g.raw(), &gt, &mt, &cam, band_ty0, band_ty1, rgba_device, aux));
    }
    // ... and with the Gaussians of `hide` culled and tint_rgba mixed into the colour of those of `tint` (gs_render_frame_sel;
    // either may be nullptr, both nullptr: the overload above)
    template <class G>
    void render(Stream &s, GaussiansBuffer<G> &g, const gs_gaussian_transform_pod &gt, const gs_model_transform_pod &mt,
                const gs_camera &cam, float *rgba_device, uint32_t band_ty0, uint32_t band_ty1, const gs_aux_targets *aux,
                const Selection *hide, const Selection *tint = nullptr, const float tint_rgba[4] = nullptr) {
        gs_frame_selection fs{};
        fs.hide = hide ? hide->raw() : nullptr;
        fs.tint = tint ? tint->raw() : nullptr;
        for (int c = 0; c < 4; c++) fs.tint_rgba[c] = tint_rgba ? tint_rgba[c] : 0.0f;
        check(gs_render_frame_sel(h_, s.raw(), g.raw(), &gt, &mt, &cam, band_ty0, band_ty1, rgba_device, aux, &fs));
    }
    // the plain or selection frame (hide / tint may be nullptr) that also ACCUMULATES its per-Gaussian contribution scores
    // into the gs_contribution records of `contrib`, at least 16 len() bytes (gs_render_frame_contrib):
    // one round, no planes; a frame never clears the records (contributions_clear)
    template <class G>
    void render_contrib(Stream &s, GaussiansBuffer<G> &g, const gs_gaussian_transform_pod &gt, const gs_model_transform_pod &mt,
                        const gs_camera &cam, float *rgba_device, Buffer &contrib, uint32_t band_ty0 = 0,
                        uint32_t band_ty1 = 0xffffffffu, const Selection *hide = nullptr, const Selection *tint = nullptr,
                        const float tint_rgba[4] = nullptr) {
        gs_frame_selection fs{};
        fs.hide = hide ? hide->raw() : nullptr;
        fs.tint = tint ? tint->raw() : nullptr;
        for (int c = 0; c < 4; c++) fs.tint_rgba[c] = tint_rgba ? tint_rgba[c] : 0.0f;
        check(gs_render_frame_contrib(h_, s.raw(), g.raw(), &gt, &mt, &cam, band_ty0, band_ty1, rgba_device, &fs, contrib.raw()));
    }
    // the Gaussians the last frame kept whose mean lies in [x0, x1) x [y0, y1) (and on a nonzero byte of the H x W device
    // plane `mask`, if given): sel = sel op that set.  Enqueued behind the frame; does not block.
    void select_visible(Stream &s, Selection &sel, float x0, float y0, float x1, float y1, const uint8_t *mask_device = nullptr,
                        gs_select_op op = GS_SEL_SET) {
        check(gs_renderer_select_visible(h_, s.raw(), sel.raw(), x0, y0, x1, y1, mask_device, op));
    }
    // render() only enqueues; wait_frame() blocks until the frame is complete and throws
    // PairCapacityError when it exceeded the pair capacity (the next frame has larger buffers)
    gs_frame_result wait_frame() { gs_frame_result fr; check(gs_renderer_wait_frame(h_, &fr)); return fr; }
    gs_frame_stats stats() { gs_frame_stats st; check(gs_renderer_stats(h_, &st)); return st; }
    // how the last frame sorted / how many rounds it took, and the pins of those per-frame choices (-1: the renderer decides;
    // every setting renders the same image; gs3d.h has the details)
    gs_sort_info sort_info() { gs_sort_info si; check(gs_renderer_sort_info(h_, &si)); return si; }
    void set_sort_mode(int32_t depth_msd, int32_t tile_msd = -1) { check(gs_renderer_set_sort_mode(h_, depth_msd, tile_msd)); }
    void set_tile_masks(int32_t mode) { check(gs_renderer_set_tile_masks(h_, mode)); }
    void set_rounds(int32_t mode, uint32_t first_round = 0) { check(gs_renderer_set_rounds(h_, mode, first_round)); }
    // sharded frames: a DEVICE word that receives every following frame's flags in stream order (nullptr: off)
    void set_frame_flags_target(uint32_t *device_word) { check(gs_renderer_set_frame_flags_target(h_, device_word)); }
  private:
    gs_renderer *h_ = nullptr;
};

// Frames in flight (no reference item: the viewer owns the frame loop; the seam is src/compute_bundle.rs:196-198 —
// dispatch only records, the caller owns the submission order).  `frames` renderers, each on a stream of its own
// PRIORITY, take the frames in turn: what a viewer with double / triple buffering does.  A frame is a chain of
// dependent kernels, latency-bound in its sorts and VALU-bound in its blend, so frames of different renderers overlap
// on the device when their streams sit on different hardware queues.  HIP keeps separate queues per priority LEVEL and
// may put streams of one level on one queue — observed, not promised: where the lanes share a queue they run one after
// the other and the ring costs what one stream costs.  Every frame is the frame its renderer would
// have rendered alone.  Presentation in order: render() returns the lane, wait(lane) blocks until THAT lane's newest
// frame is complete (lanes complete out of order when frames differ in cost).
class FrameRing {
  public:
    explicit FrameRing(Device &d, size_t frames = 3) {
        int32_t least = 0, greatest = 0;
        check(gs_device_stream_priority_range(d.raw(), &least, &greatest));
        const int32_t cycle3[3] = {greatest, least, 0};
        if (frames == 0) frames = 1;
        for (size_t k = 0; k < frames; k++) {
            const int32_t prio = least != greatest ? cycle3[k % 3] : 0;
            priorities_.push_back(prio);
            streams_.push_back(std::make_unique<Stream>(d, (int)prio));
            renderers_.push_back(std::make_unique<Renderer>(d));
        }
    }
    size_t size() const { return renderers_.size(); }
    // enqueues one frame on the next lane and returns the lane (its stream: stream(lane))
    template <class G>
    size_t render(GaussiansBuffer<G> &g, const gs_gaussian_transform_pod &gt, const gs_model_transform_pod &mt, const gs_camera &cam,
                  float *rgba_device, uint32_t band_ty0 = 0, uint32_t band_ty1 = 0xffffffffu) {
        const size_t lane = next_++ % renderers_.size();
        renderers_[lane]->render(*streams_[lane], g, gt, mt, cam, rgba_device, band_ty0, band_ty1);
        return lane;
    }
    // the same with the lane's own depth / pick planes (a lane writes them while the next lanes run)
    template <class G>
    size_t render(GaussiansBuffer<G> &g, const gs_gaussian_transform_pod &gt, const gs_model_transform_pod &mt, const gs_camera &cam,
                  float *rgba_device, uint32_t band_ty0, uint32_t band_ty1, const gs_aux_targets *aux) {
        const size_t lane = next_++ % renderers_.size();
        renderers_[lane]->render(*streams_[lane], g, gt, mt, cam, rgba_device, band_ty0, band_ty1, aux);
        return lane;
    }
    // blocks until the newest frame of `lane` is complete; throws as Renderer::wait_frame does
    gs_frame_result wait(size_t lane) { return renderers_.at(lane)->wait_frame(); }
    void synchronize() { for (auto &s : streams_) s->synchronize(); }
    Stream &stream(size_t lane) { return *streams_.at(lane); }
    Renderer &renderer(size_t lane) { return *renderers_.at(lane); }
    int32_t priority(size_t lane) const { return priorities_.at(lane); }
  private:
    // (renderers are destroyed before their streams: gs_renderer_destroy synchronises the stream of its last frame)
    std::vector<std::unique_ptr<Stream>> streams_;
    std::vector<std::unique_ptr<Renderer>> renderers_;
    std::vector<int32_t> priorities_;
    size_t next_ = 0;
};

// HIP version of the headers the library was compiled with / of the runtime / of the driver it runs on
struct HipVersions { int32_t compiled, runtime, driver; };
inline HipVersions hip_versions() { HipVersions v{0, 0, 0}; gs_hip_versions(&v.compiled, &v.runtime, &v.driver); return v; }

// G::from_gaussian on the device: `count` struct Gaussian records in `gaussians` -> PODs in `pods`
template <class G>
inline void pack_device(Device &d, Stream &s, const Buffer &gaussians, size_t count, Buffer &pods) {
    check(gs_pack_device(d.raw(), s.raw(), G::sh, G::cov3d, static_cast<const gs_gaussian *>(gaussians.device_ptr()), count,
                         pods.device_ptr()));
}

// Two device images (H x W x 4 float each, 16-byte aligned; e.g. two rgba_out_device targets) compared on the device
// (gs3d.h gs_image_compare; no reference item): error sums, maxima and counts per channel and, with
// desc.flags = GS_COMPARE_SSIM, the sums of the per-pixel SSIM.  desc == nullptr: no SSIM, L = 1, no planes.  Blocking.
inline gs_image_metrics image_compare(Device &d, Stream &s, const float *a, const float *b, uint32_t width, uint32_t height,
                                      const gs_image_compare_desc *desc = nullptr) {
    gs_image_metrics out;
    check(gs_image_compare(d.raw(), s.raw(), a, b, width, height, desc, &out));
    return out;
}
// what a caller derives from the record: the mean squared error over r g b, its PSNR (infinity at 0), the mean SSIM
inline double image_mse_rgb(const gs_image_metrics &m) { return ((m.sum_sq[0] + m.sum_sq[1]) + m.sum_sq[2]) / (3.0 * (double)m.finite); }
inline double image_psnr(const gs_image_metrics &m, double data_range = 1.0) {
    const double e = image_mse_rgb(m);
    return e == 0.0 ? std::numeric_limits<double>::infinity() : 10.0 * std::log10(data_range * data_range / e);
}
inline double image_ssim(const gs_image_metrics &m) {
    return ((m.ssim_sum[0] / (double)m.ssim_finite[0] + m.ssim_sum[1] / (double)m.ssim_finite[1]) + m.ssim_sum[2] / (double)m.ssim_finite[2]) / 3.0;
}

// ---- fast gzip members (gs3d.h gs_gzip_fast ...; no reference item) ------------------------------------
// A Huffman-only gzip member, one DEFLATE block per 32768 bytes: the host encoder, the device encoder over the bytes of a
// Buffer (Buffer::gzip_fast) and the .spz image of a GaussiansBuffer deflated where its payload is built
// (GaussiansBuffer::export_spz_fast) give the same bytes for the same input.  Each is one call into a vector of
// gs_gzip_fast_bound bytes: a size query would encode twice.  Blocking.
template <class F, class... A>
inline std::vector<uint8_t> gzip_fast_bounded(size_t input_bytes, F fn, A... head) {
    std::vector<uint8_t> out(gs_gzip_fast_bound(input_bytes));
    size_t n = 0;
    check(fn(head..., out.data(), out.size(), &n));
    out.resize(n);
    return out;
}
inline std::vector<uint8_t> gzip_fast(const void *bytes, size_t len) { return gzip_fast_bounded(len, gs_gzip_fast, bytes, len); }
inline std::vector<uint8_t> Buffer::gzip_fast(Stream &s, size_t offset, size_t len) const {
    return gzip_fast_bounded(len < size() ? len : size(), gs_buffer_gzip_fast, h_, s.raw(), offset, len);
}
template <class G>
inline std::vector<uint8_t> GaussiansBuffer<G>::export_spz_fast(Stream &s, const Selection *sel, bool invert, const gs_spz_options *options) const {
    size_t payload = 0;      // from the scan alone
    check(gs_gaussians_buffer_export_spz_decompressed(h_, s.raw(), sel ? sel->raw() : nullptr, invert ? 1 : 0, options, nullptr, 0, &payload));
    return gzip_fast_bounded(payload, gs_gaussians_buffer_export_spz_fast, h_, s.raw(), sel ? sel->raw() : nullptr, (int32_t)(invert ? 1 : 0), options);
}

}  // namespace gs3d
