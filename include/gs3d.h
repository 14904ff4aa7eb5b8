/*
 * gs3d.h — C ABI of the MI355X-native 3D Gaussian Splatting core (libgs3d_hip.so).
 *
 * This is the drop-in boundary for LioQing/wgpu-3dgs-core's render-side API: every entry point
 * names the reference interface it replaces (paths relative to the reference repository root).
 * A Rust `extern "C"` block binds these 1:1; there are no C++/torch types in any
 * signature — only opaque handles, plain pointers and sizes.
 *
 * Conventions
 *   - Every function that can fail returns gs_status (0 = GS_OK, negative = error).  The variant
 *     fields of the matching Rust error enum (src/error.rs) are available, per thread, from
 *     gs_last_error().
 *   - Handles are created/destroyed explicitly.  A handle must not be used from two threads at
 *     once; distinct handles are independent.
 *   - Every launch takes a gs_stream (a hipStream_t): the analogue of the reference's
 *     CommandEncoder + queue.submit (src/compute_bundle.rs:114-132).  Work is asynchronous
 *     unless the function is documented as blocking.
 *   - There is no CPU fallback: without a HIP device gs_device_create fails with
 *     GS_ERR_NO_DEVICE and nothing else can be constructed.
 */
#ifndef GS3D_H
#define GS3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS3D_ABI_VERSION 1

typedef int32_t gs_status;

enum {
    GS_OK = 0,
    GS_ERR_INVALID_ARGUMENT = -1,
    GS_ERR_NO_DEVICE = -2,
    GS_ERR_HIP = -3,
    GS_ERR_OUT_OF_MEMORY = -4,
    /* GaussiansBufferUpdateError::CountMismatch{count, expected_count}      src/error.rs:66-70  */
    GS_ERR_COUNT_MISMATCH = -10,
    /* GaussiansBufferUpdateRangeError::CountMismatch{count,start,expected}  src/error.rs:73-81  */
    GS_ERR_RANGE_COUNT_MISMATCH = -11,
    /* GaussiansBufferTryFromBufferError::BufferSizeNotMultiple              src/error.rs:85-94  */
    GS_ERR_BUFFER_SIZE_NOT_MULTIPLE = -12,
    /* FixedSizeBufferWrapperError::BufferSizeMismatched                     src/error.rs:97-104 */
    GS_ERR_BUFFER_SIZE_MISMATCHED = -13,
    /* ComputeBundleCreateError::ResourceCountMismatch                       src/error.rs:109-117 */
    GS_ERR_RESOURCE_COUNT_MISMATCH = -14,
    /* ComputeBundleCreateError::WorkgroupSizeExceedsDeviceLimit             src/error.rs:118-125 */
    GS_ERR_WORKGROUP_SIZE_EXCEEDS_LIMIT = -15,
    /* ComputeBundleBuildError::{MissingBindGroupLayout, MissingResolver, MissingEntryPoint,
     * MissingMainShader, Wesl}                                              src/error.rs:129-143 */
    GS_ERR_MISSING_BIND_GROUP_LAYOUT = -16,
    GS_ERR_MISSING_RESOLVER = -17,
    GS_ERR_MISSING_ENTRY_POINT = -18,
    GS_ERR_MISSING_MAIN_SHADER = -19,
    GS_ERR_KERNEL_COMPILE = -20,
    /* the reference panics: gaussian_config.rs:131-133, 211-213, 230-232 */
    GS_ERR_LOSSY_CONFIG = -21,
    /* DownloadBufferError                                                   src/error.rs:55-63  */
    GS_ERR_DOWNLOAD = -22,
    /* the frame needs more than 2^32 (tile, Gaussian) pairs: pair indices are 32-bit */
    GS_ERR_PAIR_OVERFLOW = -23,
    /* std::io::Error (InvalidData / UnexpectedEof) of the PLY reader; message = the Rust message */
    GS_ERR_PLY = -24,
    /* std::io::Error of the SPZ reader / header validation; message = the Rust message */
    GS_ERR_SPZ = -25,
    /* gs_renderer_wait_frame: the frame produced more (tile, Gaussian) pairs than the renderer's pair
     * buffers hold (a = pairs, b = capacity).  The frame was SKIPPED: the image was not written (it
     * keeps what it held) rather than blended without its farthest pairs.  The next frame grows the
     * buffers: render again.
     * A two-round frame (gs_renderer_set_rounds) bounds each ROUND on its own, usually far below the
     * buffers' capacity; a = the true pair count of the round that outgrew the bound (round 1 if both
     * did), b = that bound, and the message names the round.  Skipped by round 1, the image was not
     * written; skipped by round 2, the frame's band of the image (and of the aux planes) holds round 1's
     * intermediate pixel state — not a frame: do not present it.  The next frame has the larger bound. */
    GS_ERR_PAIR_CAPACITY = -26,
    /* gs_renderer_wait_frame: the watchdog of the radix sort's LDS-atomic rank fired in this frame (an order
     * assumption about returning LDS atomics that the hardware documents do not promise; probed at
     * gs_device_create and checked by block 0 of every pass).  The frame's blend order may be wrong; the device
     * has been switched to the ballot-based rank for good: render again. */
    GS_ERR_RANK_ORDER = -27
};

/* Thread-local details of the last failing call on this thread.
 *   COUNT_MISMATCH:            a = count, b = expected_count
 *   RANGE_COUNT_MISMATCH:      a = count, b = start, c = expected_count
 *   BUFFER_SIZE_NOT_MULTIPLE:  a = buffer_size, b = expected_multiple_size
 *   BUFFER_SIZE_MISMATCHED:    a = buffer_size, b = expected_size
 *   RESOURCE_COUNT_MISMATCH:   a = resource_count, b = bind_group_layout_count
 *   WORKGROUP_SIZE_EXCEEDS_LIMIT: a = workgroup_size, b = device_limit
 *   HIP:                       a = hipError_t                                                   */
typedef struct gs_error_info {
    int32_t code;
    uint64_t a, b, c;
    char message[256];
} gs_error_info;

void gs_last_error(gs_error_info *out);
const char *gs_status_string(gs_status s);
uint32_t gs_abi_version(void);
/* wgpu::Adapter::get_info() analogue (AdapterInfo::driver_info): the HIP version this library was
 * COMPILED against (HIP_VERSION of the headers) and the versions of the runtime and driver it is
 * RUNNING on (hipRuntimeGetVersion / hipDriverGetVersion; 0 when the call fails).  A Python host that
 * also imports PyTorch runs the library on the runtime bundled with the torch wheel, which may be older
 * than the headers: every benchmark record prints both. */
void gs_hip_versions(int32_t *compiled, int32_t *runtime, int32_t *driver);

/* ------------------------------------------------------------------------------------------ */
/* Data model                                                                                  */
/* ------------------------------------------------------------------------------------------ */

/* GaussianShConfig / GaussianCov3dConfig families — src/gaussian_config.rs:15-233 */
typedef enum { GS_SH_SINGLE = 0, GS_SH_HALF = 1, GS_SH_NORM8 = 2, GS_SH_NONE = 3 } gs_sh_config;
typedef enum { GS_COV3D_ROT_SCALE = 0, GS_COV3D_SINGLE = 1, GS_COV3D_HALF = 2 } gs_cov3d_config;

/* struct Gaussian — src/gaussian.rs:53-60 (rot = xyzw; 224 bytes) */
typedef struct gs_gaussian {
    float rot[4];
    float pos[3];
    uint8_t color[4];
    float sh[45];
    float scale[3];
} gs_gaussian;

/* GaussianDisplayMode — src/buffer/gaussian_transform.rs:7-14 */
typedef enum { GS_DISPLAY_SPLAT = 0, GS_DISPLAY_ELLIPSE = 1, GS_DISPLAY_POINT = 2 } gs_display_mode;

/* GaussianTransformPod — src/buffer/gaussian_transform.rs:166-174 (8 bytes) */
typedef struct gs_gaussian_transform_pod {
    float size;
    uint8_t flags[4]; /* display_mode, sh_deg, no_sh0, max_std_dev (u8) */
} gs_gaussian_transform_pod;

/* ModelTransformPod — src/buffer/model_transform.rs:61-66 (48 bytes) */
typedef struct gs_model_transform_pod {
    float pos[3];
    float _pad0;
    float rot[4];
    float scale[3];
    float _pad1;
} gs_model_transform_pod;

/* std::mem::size_of::<GaussianPodWithSh{S}Cov3d{C}Configs>() — src/buffer/gaussian.rs:373-384 */
size_t gs_pod_size(gs_sh_config sh, gs_cov3d_config cov);
/* GaussianPod::features() — src/buffer/gaussian.rs:270-286; order: sh_single, sh_half, sh_norm8,
 * sh_none, cov3d_rot_scale, cov3d_single, cov3d_half */
gs_status gs_pod_features(gs_sh_config sh, gs_cov3d_config cov, uint8_t out[7]);
const char *gs_feature_name(uint32_t index);
/* G::from_gaussian — src/buffer/gaussian.rs:314-339 (host, multi-threaded) */
gs_status gs_pack(gs_sh_config sh, gs_cov3d_config cov, const gs_gaussian *in, size_t n, void *out);
/* Into<Gaussian> — src/buffer/gaussian.rs:341-363; GS_ERR_LOSSY_CONFIG where Rust panics */
gs_status gs_unpack_to_gaussian(gs_sh_config sh, gs_cov3d_config cov, const void *pods, size_t n,
                                gs_gaussian *out);

/* GaussianShDegree::new / GaussianMaxStdDev::new / GaussianTransformPod::new —
 * src/buffer/gaussian_transform.rs:25-30, 63-68, 178-194.  GS_ERR_INVALID_ARGUMENT where the
 * Rust constructors return None. */
gs_status gs_gaussian_transform_pod_new(float size, gs_display_mode mode, uint8_t sh_deg,
                                        uint8_t no_sh0, float max_std_dev,
                                        gs_gaussian_transform_pod *out);
void gs_gaussian_transform_pod_default(gs_gaussian_transform_pod *out);
gs_status gs_max_std_dev_encode(float max_std_dev, uint8_t *out);
float gs_max_std_dev_decode(uint8_t v);
/* ModelTransformPod::new / default — src/buffer/model_transform.rs:68-84 */
void gs_model_transform_pod_new(const float pos[3], const float rot_xyzw[4], const float scale[3],
                                gs_model_transform_pod *out);
void gs_model_transform_pod_default(gs_model_transform_pod *out);

/* ------------------------------------------------------------------------------------------ */
/* Inria PLY source format — src/source_format/ply.rs, src/gaussian.rs:70-125 (host side)      */
/* ------------------------------------------------------------------------------------------ */

/* PlyGaussianPod — src/source_format/ply.rs:11-21 (62 little-endian f32 = 248 bytes) */
typedef struct gs_ply_gaussian_pod {
    float pos[3];
    float normal[3];
    float color[3];   /* f_dc_0..2 */
    float sh[45];     /* f_rest_0..44, channel-planar */
    float alpha;      /* opacity (logit) */
    float scale[3];   /* log scale */
    float rot[4];     /* wxyz */
} gs_ply_gaussian_pod;

/* PlyGaussians::PLY_PROPERTIES — ply.rs:204-267 */
const char *gs_ply_property_name(uint32_t index);
/* Gaussian::from_ply / Gaussian::to_ply — src/gaussian.rs:70-125 */
void gs_gaussian_from_ply(const gs_ply_gaussian_pod *in, size_t n, gs_gaussian *out);
/* The exp of Gaussian::from_ply (f32::exp in the reference, src/gaussian.rs:76,81): the double-based
 * table algorithm glibc's expf uses, restated so that the host path above and the device path
 * (gs_pack_device_from_ply) give the same bits (csrc/gs_convert.h). */
float gs_expf(float x);
/* The ln of Gaussian::to_ply / to_spz (f32::ln in the reference, src/gaussian.rs:100,105,254): the double-based table
 * algorithm glibc's logf uses, restated so that the host paths (gs_gaussian_to_ply, gs_spz_encode_decompressed) and the device
 * path (gs_gaussians_buffer_export_*) give the same bits (csrc/gs_convert.h).  Bit-equal to glibc 2.35's logf for every
 * binary32 input: -inf for +-0, 0xffc00000 for a negative argument, the argument quieted for a NaN. */
float gs_logf(float x);
void gs_gaussian_to_ply(const gs_gaussian *in, size_t n, gs_ply_gaussian_pod *out);
/* PlyGaussians::read_from — ply.rs:292-408.  Call with out == NULL to get the vertex count, then
 * with a buffer.  Handles the Inria fast path (one memcpy) and custom property orders in ascii /
 * binary little / big endian.  Errors: GS_ERR_PLY with the reference's message, e.g.
 * "Gaussian vertex element not found in PLY header",
 * "Gaussian element property invalid or missing in PLY". */
gs_status gs_ply_read(const void *bytes, size_t len, gs_ply_gaussian_pod *out, size_t capacity,
                      size_t *count_out, int32_t *is_inria_out);
/* PlyGaussians::write_to — ply.rs:410-431 (binary_little_endian Inria layout).  Call with
 * out == NULL to get the size. */
gs_status gs_ply_write(const gs_ply_gaussian_pod *pods, size_t n, void *out, size_t capacity,
                       size_t *bytes_out);

/* ------------------------------------------------------------------------------------------ */
/* SPZ source format — src/source_format/spz.rs, src/gaussian.rs:126-352 (host side)           */
/* ------------------------------------------------------------------------------------------ */

/* SpzGaussiansHeaderPod — spz.rs:436-446 (16 bytes; magic 0x5053474e, versions 1..=3) */
typedef struct gs_spz_header {
    uint32_t magic;
    uint32_t version;
    uint32_t num_points;
    uint8_t sh_degree;
    uint8_t fractional_bits;
    uint8_t flags;      /* bit 0 = antialiased */
    uint8_t reserved;
} gs_spz_header;

/* SpzGaussiansFromGaussianSliceOptions — spz.rs:962-999 (default: version 3, sh 3, 12 fractional
 * bits, not antialiased, sh_quantize_bits [5,4,4]) */
typedef struct gs_spz_options {
    uint32_t version;
    uint8_t sh_degree;
    uint8_t fractional_bits;
    uint8_t antialiased;
    uint8_t _pad;
    uint32_t sh_quantize_bits[3];
} gs_spz_options;

void gs_spz_options_default(gs_spz_options *out);
/* SpzGaussians::read_from + iter_gaussian (gzip -> columns -> Gaussian::from_spz).  Call with
 * out == NULL for the count / header.  Errors: GS_ERR_SPZ with the reference's message, e.g.
 * "Invalid SPZ magic number: 0, expected 5053474E", "Unsupported SPZ version: 999, expected one of 1..=3" */
gs_status gs_spz_decode(const void *bytes, size_t len, gs_spz_header *header_out, gs_gaussian *out,
                        size_t capacity, size_t *count_out);
gs_status gs_spz_decode_decompressed(const void *bytes, size_t len, gs_spz_header *header_out,
                                     gs_gaussian *out, size_t capacity, size_t *count_out);
/* SpzGaussians::from_gaussians_with_options + write_to (Gaussian::to_spz -> columns -> gzip).
 * Call with out == NULL for the size. */
gs_status gs_spz_encode(const gs_gaussian *in, size_t n, const gs_spz_options *options, void *out,
                        size_t capacity, size_t *bytes_out);
gs_status gs_spz_encode_decompressed(const gs_gaussian *in, size_t n, const gs_spz_options *options,
                                     void *out, size_t capacity, size_t *bytes_out);
/* the gzip member around the payload on its own (flate2 GzDecoder / GzEncoder, spz.rs:945-959), so a
 * host mirror can keep the payload it read and write the identical columns back.  out == NULL: size */
gs_status gs_spz_decompress(const void *bytes, size_t len, void *out, size_t capacity, size_t *bytes_out);
gs_status gs_spz_compress(const void *bytes, size_t len, void *out, size_t capacity, size_t *bytes_out);

/* GaussiansSource / Gaussians — src/gaussian.rs:394-548: the unified representation, reduced to
 * what crosses an FFI: read a source format into Gaussians, write Gaussians as a source format.
 *   gs_gaussians_read  = Gaussians::read_from(reader, source)?.iter_gaussian()   (:478-497)
 *   gs_gaussians_write = Gaussians::from_gaussians_iter(iter, source).write_to(writer)   (:426-436, 513-524;
 *                        SPZ with the default options, as `iter.collect::<SpzGaussians>()` does)
 * GS_SOURCE_INTERNAL fails with the reference's InvalidInput messages ("cannot read Internal
 * Gaussians from buffer" / "cannot write Internal Gaussians to buffer") as GS_ERR_INVALID_ARGUMENT.
 * Call with out == NULL for the count / size. */
typedef enum { GS_SOURCE_INTERNAL = 0, GS_SOURCE_PLY = 1, GS_SOURCE_SPZ = 2 } gs_gaussians_source;
gs_status gs_gaussians_read(const void *bytes, size_t len, gs_gaussians_source source, gs_gaussian *out,
                            size_t capacity, size_t *count_out);
gs_status gs_gaussians_write(const gs_gaussian *in, size_t n, gs_gaussians_source source, void *out,
                             size_t capacity, size_t *bytes_out);

/* ------------------------------------------------------------------------------------------ */
/* Device, streams                                                                             */
/* ------------------------------------------------------------------------------------------ */

typedef struct gs_device gs_device;   /* wgpu::Device + wgpu::Queue */
typedef struct gs_stream gs_stream;   /* wgpu::CommandEncoder + queue.submit */

/* wgpu::Limits fields read by src/compute_bundle.rs:269-272 */
typedef struct gs_limits {
    uint32_t max_compute_workgroup_size_x;
    uint32_t max_compute_invocations_per_workgroup;
    uint32_t compute_units;
    uint32_t wavefront_size;
    uint64_t total_memory_bytes;
    char arch_name[64];
} gs_limits;

gs_status gs_device_create(int32_t hip_ordinal, gs_device **out);
void gs_device_destroy(gs_device *dev);
gs_status gs_device_limits(const gs_device *dev, gs_limits *out);
gs_status gs_device_synchronize(gs_device *dev);
/* 1 while the radix sorts of this device rank with returning LDS atomics (the order probe of gs_device_create passed
 * and the per-frame watchdog has not fired: GS_ERR_RANK_ORDER), 0 once they use the ballot-based rank (no reference
 * item: wgpu has no such primitive) */
int32_t gs_device_fast_rank(const gs_device *dev);
gs_status gs_stream_create(gs_device *dev, gs_stream **out);
/* Streams of one process that should run CONCURRENTLY on the device (two frames in flight: the latency-bound sort
 * chain of frame i + 1 under the VALU-bound blend of frame i) must sit on different hardware queues; HIP gives every
 * priority level its own queues, and streams of equal priority may share one (measured under torch: they do).
 * priority: hipStreamCreateWithPriority's number, between *least and *greatest of gs_device_stream_priority_range
 * (numerically lower = higher priority).  No reference item: a wgpu::Queue has no priority. */
gs_status gs_stream_create_with_priority(gs_device *dev, int32_t priority, gs_stream **out);
gs_status gs_device_stream_priority_range(gs_device *dev, int32_t *least, int32_t *greatest);
/* borrow an existing hipStream_t (e.g. the stream a caller's framework is using) */
gs_status gs_stream_wrap(gs_device *dev, void *hip_stream, gs_stream **out);
void *gs_stream_native(const gs_stream *s);
gs_status gs_stream_synchronize(gs_stream *s);
/* Lifetime: a renderer whose newest frame was enqueued on `s` stays usable — gs_stream_destroy records that frame's end
 * event on the stream before it goes, and later frames / waits of the renderer are ordered behind the event, not the
 * stream.  A WRAPPED stream (gs_stream_wrap) must therefore be handed to gs_stream_destroy BEFORE the caller destroys
 * the hipStream_t it wraps. */
void gs_stream_destroy(gs_stream *s);

/* ------------------------------------------------------------------------------------------ */
/* Buffers — trait BufferWrapper / FixedSizeBufferWrapper, src/buffer/mod.rs:17-150            */
/* ------------------------------------------------------------------------------------------ */

typedef struct gs_buffer gs_buffer; /* wgpu::Buffer: ref-counted device allocation */

gs_status gs_buffer_create(gs_device *dev, size_t bytes, const void *init_or_null, gs_buffer **out);
/* adopt device memory the caller owns (non-owning; the TryFrom<wgpu::Buffer> direction) */
gs_status gs_buffer_from_raw(gs_device *dev, void *device_ptr, size_t bytes, gs_buffer **out);
gs_buffer *gs_buffer_retain(gs_buffer *b); /* Clone = handle copy (buffer/gaussian.rs:16) */
void gs_buffer_release(gs_buffer *b);
size_t gs_buffer_size(const gs_buffer *b);
void *gs_buffer_device_ptr(const gs_buffer *b);
/* queue.write_buffer(buffer, offset, data) */
gs_status gs_buffer_write(gs_buffer *b, gs_stream *s, size_t offset, const void *src, size_t bytes);
/* BufferWrapper::download — src/buffer/mod.rs:27-42 (blocking: prepare_download + map + poll) */
gs_status gs_buffer_download(gs_buffer *b, gs_stream *s, void *dst, size_t bytes);
/* BufferWrapper::prepare_download — src/buffer/mod.rs:48-78: enqueues the copy of the whole buffer
 * into a host-visible staging buffer on `s` and returns at once (the wgpu original records
 * copy_buffer_to_buffer into the caller's encoder).
 * BufferWrapper::map_download — :80-101: gs_download_map blocks until the copy has landed (the
 * map_async + device.poll(wait) of the original) and exposes the bytes, valid until
 * gs_download_release; gs_download_ready polls without blocking.
 * Errors: GS_ERR_DOWNLOAD (DownloadBufferError). */
typedef struct gs_download gs_download;
gs_status gs_buffer_prepare_download(gs_buffer *b, gs_stream *s, gs_download **out);
int32_t gs_download_ready(gs_download *d);
gs_status gs_download_map(gs_download *d, const void **data_out, size_t *bytes_out);
void gs_download_release(gs_download *d);

/* GaussiansBuffer<G> — src/buffer/gaussian.rs:17-229 */
typedef struct gs_gaussians_buffer gs_gaussians_buffer;

/* new_with_pods (pods != NULL) / new_empty (pods == NULL) — :50-90 */
gs_status gs_gaussians_buffer_create(gs_device *dev, gs_sh_config sh, gs_cov3d_config cov,
                                     const void *pods_or_null, size_t len,
                                     gs_gaussians_buffer **out);
/* new(device, gaussians): upload the source records, pack on the device (gs_pack_device) — :21-30 */
gs_status gs_gaussians_buffer_create_from_gaussians(gs_device *dev, gs_sh_config sh,
                                                    gs_cov3d_config cov, const gs_gaussian *gaussians,
                                                    size_t len, gs_gaussians_buffer **out);
/* PlyGaussians -> GaussiansBuffer in one step: the 248-byte vertex records cross PCIe as they are (one
 * copy per slice) and ONE kernel does Gaussian::from_ply (src/gaussian.rs:70-92) fused with
 * G::from_gaussian (src/buffer/gaussian.rs:314-339) — what the reference does per vertex on the host
 * (src/source_format/ply.rs:386-390 iter_gaussian + src/buffer/gaussian.rs:21-30 new).  The PODs are
 * bit-equal to gs_gaussian_from_ply followed by gs_pack. */
gs_status gs_gaussians_buffer_create_from_ply(gs_device *dev, gs_sh_config sh, gs_cov3d_config cov,
                                              const gs_ply_gaussian_pod *ply, size_t len,
                                              gs_gaussians_buffer **out);
/* the same for [start, start + count) of an existing buffer (update_range semantics and errors) */
gs_status gs_gaussians_buffer_update_range_ply(gs_gaussians_buffer *g, gs_stream *s, size_t start,
                                               const gs_ply_gaussian_pod *ply, size_t count);
/* SpzGaussians -> GaussiansBuffer: inflate on the host (a gzip member is sequential), then the
 * decompressed columns cross PCIe once and ONE kernel does Gaussian::from_spz
 * (src/gaussian.rs:134-229 over spz.rs:739-771's columns) fused with G::from_gaussian.  The PODs are
 * bit-equal to gs_spz_decode followed by gs_pack; errors as gs_spz_decode (GS_ERR_SPZ). */
gs_status gs_gaussians_buffer_create_from_spz(gs_device *dev, gs_sh_config sh, gs_cov3d_config cov,
                                              const void *bytes, size_t len, gs_spz_header *header_out,
                                              gs_gaussians_buffer **out);
gs_status gs_gaussians_buffer_create_from_spz_decompressed(gs_device *dev, gs_sh_config sh, gs_cov3d_config cov,
                                                           const void *bytes, size_t len,
                                                           gs_spz_header *header_out,
                                                           gs_gaussians_buffer **out);
/* the kernel itself: `n` PlyGaussianPod records in DEVICE memory -> PODs in device memory */
gs_status gs_pack_device_from_ply(gs_device *dev, gs_stream *s, gs_sh_config sh, gs_cov3d_config cov,
                                  const gs_ply_gaussian_pod *ply_device, size_t n, void *pods_device);
/* TryFrom<wgpu::Buffer> — :213-229; the wrapper retains `buffer` */
/* G::from_gaussian on the device (src/buffer/gaussian.rs:314-339 for all 12 PODs): `n` source
 * records (struct Gaussian, 224 bytes each) already in device memory -> PODs in device memory, bit-equal
 * to gs_pack.  GaussiansBuffer::new / update / update_range with Gaussians go through this: the
 * source records cross PCIe once and are packed on the device. */
gs_status gs_pack_device(gs_device *dev, gs_stream *s, gs_sh_config sh, gs_cov3d_config cov,
                         const gs_gaussian *gaussians_device, size_t n, void *pods_device);
gs_status gs_gaussians_buffer_from_buffer(gs_buffer *buffer, gs_sh_config sh, gs_cov3d_config cov,
                                          gs_gaussians_buffer **out);
void gs_gaussians_buffer_destroy(gs_gaussians_buffer *g);
size_t gs_gaussians_buffer_len(const gs_gaussians_buffer *g); /* :93-95 */
gs_buffer *gs_gaussians_buffer_buffer(const gs_gaussians_buffer *g); /* BufferWrapper::buffer(), borrowed */
gs_sh_config gs_gaussians_buffer_sh(const gs_gaussians_buffer *g);
gs_cov3d_config gs_gaussians_buffer_cov3d(const gs_gaussians_buffer *g);
/* update_with_pod — :122-138 */
gs_status gs_gaussians_buffer_update(gs_gaussians_buffer *g, gs_stream *s, const void *pods,
                                     size_t count);
/* update_range_with_pod — :161-183 */
gs_status gs_gaussians_buffer_update_range(gs_gaussians_buffer *g, gs_stream *s, size_t start,
                                           const void *pods, size_t count);
/* update / update_range with Gaussians (host pack first) — :103-118, :143-158 */
gs_status gs_gaussians_buffer_update_gaussians(gs_gaussians_buffer *g, gs_stream *s,
                                               const gs_gaussian *gaussians, size_t count);
gs_status gs_gaussians_buffer_update_range_gaussians(gs_gaussians_buffer *g, gs_stream *s,
                                                     size_t start, const gs_gaussian *gaussians,
                                                     size_t count);
/* download::<G> (pods) and download_gaussians — :186-195 (blocking).  download_gaussians converts
 * POD -> Gaussian (GaussianPod::into_gaussian) on the DEVICE and copies struct Gaussian records back;
 * GS_ERR_LOSSY_CONFIG for ShNone / Cov3dSingle / Cov3dHalf, where the reference panics. */
gs_status gs_gaussians_buffer_download(gs_gaussians_buffer *g, gs_stream *s, void *pods_out,
                                       size_t count);
gs_status gs_gaussians_buffer_download_gaussians(gs_gaussians_buffer *g, gs_stream *s,
                                                 gs_gaussian *out, size_t count);
/* tell the wrapper that device code wrote the underlying buffer (e.g. a compute bundle bound it
 * read-write), so the renderer's block-planar mirror must be rebuilt on the next frame */
void gs_gaussians_buffer_mark_dirty(gs_gaussians_buffer *g);
/* The renderer reads a mirror of the buffer whose slots are, by default, in SPATIAL order: ids
 * sorted by the 30-bit Morton code of the position (10 bits per axis over the bounding box of all
 * positions; ties by index) — DESIGN.md §3.4a.  The order is computed whenever the whole buffer
 * is (re)mirrored (creation, gs_gaussians_buffer_update, mark_dirty); update_range keeps it.  It is
 * observable in exactly one way: (tile, Gaussian) pairs with bit-identical depth in one tile are
 * blended in mirror order.  Disable (index order) per buffer here or globally with
 * GS3D_SPATIAL_ORDER=0.  download_order writes order[slot] = Gaussian index (the identity when
 * disabled); count must equal the buffer length. */
gs_status gs_gaussians_buffer_set_spatial_order(gs_gaussians_buffer *g, int32_t enabled);
int32_t gs_gaussians_buffer_spatial_order(const gs_gaussians_buffer *g);
gs_status gs_gaussians_buffer_download_order(gs_gaussians_buffer *g, gs_stream *s, uint32_t *order_out,
                                             size_t count);

/* GaussianTransformBuffer — src/buffer/gaussian_transform.rs:104-163 (8-byte uniform) */
gs_status gs_gaussian_transform_buffer_create(gs_device *dev, gs_buffer **out);
gs_status gs_gaussian_transform_buffer_update(gs_buffer *b, gs_stream *s,
                                              const gs_gaussian_transform_pod *pod);
gs_status gs_gaussian_transform_buffer_from_buffer(gs_buffer *b); /* size check only */
/* ModelTransformBuffer — src/buffer/model_transform.rs:10-58 (48-byte uniform) */
gs_status gs_model_transform_buffer_create(gs_device *dev, gs_buffer **out);
gs_status gs_model_transform_buffer_update(gs_buffer *b, gs_stream *s,
                                           const gs_model_transform_pod *pod);
gs_status gs_model_transform_buffer_from_buffer(gs_buffer *b);

/* ------------------------------------------------------------------------------------------ */
/* ComputeBundle — src/compute_bundle.rs:49-351                                                */
/* ------------------------------------------------------------------------------------------ */

/* The kernel registry replaces shader::PACKAGE + wesl feature flags (src/shader.rs:8-56):
 * "features" select a template instantiation keyed by (sh, cov). */
typedef enum {
    /* tests/common/shader/array_map_add.wesl: group0 = {data rw u32[]}, group1 = {uniform u32};
     * data[i] += uniform + constant("add_constant") */
    GS_KERNEL_ARRAY_MAP_ADD = 0,
    /* tests/shader/gaussian.rs:26-59: group0 = {gaussians, output(56 f32)} */
    GS_KERNEL_TEST_GAUSSIAN = 1,
    /* tests/shader/gaussian_transform.rs:13-48: group0 = {transform uniform, output(4 u32)} */
    GS_KERNEL_TEST_GAUSSIAN_TRANSFORM = 2,
    /* tests/shader/model_transform.rs:14-51: group0 = {model uniform, output(38 f32)} */
    GS_KERNEL_TEST_MODEL_TRANSFORM = 3,
    /* AoS pods -> SoA f32 planes (color4, sh45, cov6) for `count` Gaussians: group0 = {gaussians, out} */
    GS_KERNEL_UNPACK_SOA = 4,
    GS_KERNEL_COUNT_ = 5
} gs_kernel_id;

typedef struct gs_bundle gs_bundle;

typedef struct gs_bundle_desc {
    const char *label;          /* may be NULL ("Compute Bundle") */
    gs_kernel_id kernel;        /* main_shader + entry_point */
    gs_sh_config sh;            /* wesl features */
    gs_cov3d_config cov;
    uint32_t bind_group_count;  /* bind_group_layouts.len() */
    const uint32_t *bindings_per_group;
    uint32_t workgroup_size;    /* 0 = None = device limit (compute_bundle.rs:274) */
    const char *const *constant_names; /* PipelineCompilationOptions.constants */
    const double *constant_values;
    uint32_t constant_count;
} gs_bundle_desc;

/* ComputeBundle::new_without_bind_groups — :260-341 */
gs_status gs_bundle_create(gs_device *dev, const gs_bundle_desc *desc, gs_bundle **out);
/* ComputeBundle::new — :141-188: `resources` = bind_group_count_given arrays of buffers;
 * GS_ERR_RESOURCE_COUNT_MISMATCH when group counts differ */
gs_status gs_bundle_create_with_bind_groups(gs_device *dev, const gs_bundle_desc *desc,
                                            gs_buffer *const *const *resources,
                                            const uint32_t *resource_counts,
                                            uint32_t resource_group_count, gs_bundle **out);
/* ComputeBundleBuilder::build with a caller-supplied shader — compute_bundle.rs:500-586.
 * `source` is HIP C++ (the MI355X replacement for the WESL main module).  It is compiled at run
 * time with hiprtc for the device's gfx arch; `#include <wgpu_3dgs_core.h>` imports the device
 * library (namespace gs: gaussian_unpack_color / _sh<SH> / _cov3d<SH,COV>, gaussian_transform_*,
 * model_*; the WESL package of src/shader.rs).  The entry point must be
 *     extern "C" __global__ void <entry_point>(gs::BundleArgs a, uint32_t count)
 * Feature flags arrive as macros: GS_SH, GS_COV (config indices) plus one macro per enabled
 * feature name (sh_single, cov3d_half, ... and every string of `defines`); the reference's
 * `override workgroup_size` is the macro `workgroup_size`; pipeline constants are macros of their
 * names.  Compilation errors -> GS_ERR_KERNEL_COMPILE (the ComputeBundleBuildError::Wesl analogue)
 * with the compiler log in gs_last_error().message. */
typedef struct gs_bundle_source_desc {
    const char *label;
    const char *source;
    const char *entry_point;
    gs_sh_config sh;
    gs_cov3d_config cov;
    uint32_t bind_group_count;
    const uint32_t *bindings_per_group;
    uint32_t workgroup_size;
    const char *const *constant_names;
    const double *constant_values;
    uint32_t constant_count;
    const char *const *defines;
    uint32_t define_count;
} gs_bundle_source_desc;
gs_status gs_bundle_create_from_source(gs_device *dev, const gs_bundle_source_desc *desc, gs_bundle **out);
/* create bind groups on a bundle built without them (`build` = `build_without_bind_groups` + this);
 * GS_ERR_RESOURCE_COUNT_MISMATCH as in compute_bundle.rs:161-168 */
gs_status gs_bundle_attach_bind_groups(gs_bundle *b, gs_buffer *const *const *resources,
                                       const uint32_t *resource_counts, uint32_t resource_group_count);
void gs_bundle_destroy(gs_bundle *b);
uint32_t gs_bundle_workgroup_size(const gs_bundle *b);
const char *gs_bundle_label(const gs_bundle *b);
uint32_t gs_bundle_bind_group_layout_count(const gs_bundle *b);
uint32_t gs_bundle_bind_group_count(const gs_bundle *b);
/* update_bind_group_with_binding_resources — :222-231; GS_ERR_INVALID_ARGUMENT when the index is
 * out of bounds (Rust returns None) */
gs_status gs_bundle_set_bind_group(gs_bundle *b, uint32_t index, gs_buffer *const *buffers,
                                   uint32_t count);
/* dispatch — :196-198: ceil(count / workgroup_size) workgroups on `s` */
gs_status gs_bundle_dispatch(gs_bundle *b, gs_stream *s, uint32_t count);
/* dispatch_with_bind_groups — :114-132 (ComputeBundle<()>::dispatch :344-351) */
gs_status gs_bundle_dispatch_with_bind_groups(gs_bundle *b, gs_stream *s, uint32_t count,
                                              gs_buffer *const *const *groups,
                                              const uint32_t *group_counts, uint32_t group_count);
/* number of workgroups the last dispatch launched (launch arithmetic check) */
uint32_t gs_bundle_last_workgroup_count(const gs_bundle *b);

/* ------------------------------------------------------------------------------------------ */
/* Render path (absent from the reference crate; see DESIGN.md §3 for its definition)          */
/* ------------------------------------------------------------------------------------------ */

/* view: column-major world->view, right-handed, camera looks down -Z, +Y up */
typedef struct gs_camera {
    float view[16];
    float pos[3];
    float fx, fy, cx, cy;
    float near_plane, far_plane;
    uint32_t width, height;
    float background[3];
} gs_camera;

/* 48-byte projected splat record; conic pre-scaled to (-A/2, -B, -C/2) */
typedef struct gs_projected {
    float mx, my;
    float ca, cb, cc;
    float opacity;
    float r, g, b;
    float depth;
    uint16_t tx0, ty0, tx1, ty1;
} gs_projected;

typedef struct gs_frame_stats {
    uint64_t gaussians;       /* N */
    uint64_t visible;         /* Gaussians with >= 1 tile */
    uint64_t pairs;           /* D = (tile, Gaussian) pairs */
    uint32_t tiles_x, tiles_y;
    uint32_t sort_passes;
    uint32_t timed_frames;    /* frames accumulated below since the last reset */
    /* accumulated stage time in ms (only while timing is enabled):
     * 0 repack, 1 preprocess + compaction of the visible Gaussians, 2 sizing pass (0 in steady
     * state), 3 depth sort, 4 pair expansion, 5 tile sort, 6 ranges, 7 blend, 8 whole frame */
    double stage_ms[12];
} gs_frame_stats;

typedef struct gs_renderer gs_renderer;

void gs_camera_look_at(const float eye[3], const float target[3], const float up[3],
                       float vfov_radians, uint32_t width, uint32_t height, float near_plane,
                       float far_plane, gs_camera *out);

gs_status gs_renderer_create(gs_device *dev, gs_renderer **out);
void gs_renderer_destroy(gs_renderer *r);
/* stage timing with HIP events on the launch stream (off by default) */
gs_status gs_renderer_set_timing(gs_renderer *r, int32_t enabled);
gs_status gs_renderer_reset_stats(gs_renderer *r);
/* Sharded frames (no reference item: the viewer owns the frame): a DEVICE word that
 * receives the flags of every following frame of this renderer (gs_frame_result.flags: bit 0 capacity exceeded, bit 1 skipped; 0 = the band was
 * rendered), written in stream order by the kernel that publishes the frame result — no extra
 * launch.  A rank points it at a word inside its chunk of the gather buffer, so the one all-gather
 * that exchanges the bands also tells every rank whether ANY band was skipped (pair capacity), and
 * the frame can be dropped as a whole instead of being shown torn.  NULL (the default) disables.
 * The word must stay valid until the frames that were enqueued with it have completed. */
gs_status gs_renderer_set_frame_flags_target(gs_renderer *r, uint32_t *device_word);
/* blocking: synchronises the stream of the last frame first */
gs_status gs_renderer_stats(gs_renderer *r, gs_frame_stats *out);

/* One frame: repack (if the Gaussians changed) -> preprocess + ordered compaction of the visible
 * Gaussians -> depth sort -> pair expansion in depth order -> stable tile sort -> tile ranges ->
 * blend.  Renders tile rows [band_ty0, band_ty1) (16-pixel rows; pass 0 and UINT32_MAX for the whole
 * image) into rgba_out_device, a device pointer to the FULL height x width x 4 f32 image (16-byte
 * aligned); only the band's rows are written.  All three GaussianDisplayModes of the transform are
 * rendered (Splat: Gaussian falloff; Ellipse: flat alpha inside the max_std_dev ellipse; Point:
 * flat alpha inside a 1.5-pixel dot — DESIGN.md §3.5a).
 *
 * (A)synchrony — the analogue of ComputeBundle::dispatch recording into a CommandEncoder that
 * executes at queue.submit (src/compute_bundle.rs:114-132): the call only ENQUEUES work on `s` and
 * returns; the image is complete when the stream has been synchronised (or gs_renderer_wait_frame
 * has returned).  The visible count V and the pair count D never come back to the host inside a
 * frame: grids are sized from host-side bounds and the kernels read V and D on the device.
 * The one exception is a SIZING frame — the first frame of a renderer, or the first after the
 * Gaussian count, image size or band changed — which blocks once in the middle to measure D and
 * size the pair buffers (GS_ERR_PAIR_OVERFLOW if D would exceed 2^32).  Later frames take the
 * capacity from the measured D of earlier frames (25 % head room over the last D, or over the last
 * step extrapolated three frames ahead while D keeps growing; grown lazily: buffer growth calls
 * hipFree, which synchronises the device).  If a frame nevertheless produces more pairs than fit, the
 * device notices before the blend and the frame is SKIPPED — the RGBA target is left untouched, no
 * image with missing splats is ever written — gs_renderer_wait_frame reports GS_ERR_PAIR_CAPACITY
 * (flags bits 0 and 1) and the next gs_render_frame has the larger buffers: a viewer that presents a
 * frame only after wait_frame / flags == 0 shows the previous frame once more, never a wrong one.
 * A two-round frame (gs_renderer_set_rounds) is skipped in the same way when one of its ROUNDS outgrows
 * the per-round bound taken from the previous two-round frame's report, with one difference: skipped
 * by its second round, the target is NOT untouched — its band holds the first round's intermediate
 * pixel state (the known defect described at gs_renderer_set_rounds).  The flags, the error and the
 * recovery in the next frame are the same, and so is the viewer's rule: present on flags == 0 only.
 *
 * Frames in flight: a renderer owns the scratch buffers of ONE frame, so consecutive frames on one
 * renderer run one after the other: in stream order on one stream, and when a frame is submitted on a
 * different stream than the renderer's previous frame it is ordered behind that frame's end-of-frame
 * event (a device-side wait, the call does not block).  To overlap frames (the sort chain of frame i + 1 fills the gaps
 * of frame i's blend: +20 % frames per second at 1 M Gaussians), use one gs_renderer per frame slot,
 * each on its own gs_stream, and hand them the frames in turn; the Gaussian buffer is shared (the
 * renderer-internal mirror of the buffer is built on the stream of the first frame that needs it and
 * frames on other streams wait for that build; UPDATING a buffer that frames on other streams may
 * still be reading is the caller's to order, as with any buffer used across streams).
 *
 * Limits (GS_ERR_INVALID_ARGUMENT beyond them): at most 2^22 tiles of 16 x 16 pixels and 65535 tiles
 * along either axis; at most 2^32 - 16 Gaussians. */
gs_status gs_render_frame(gs_renderer *r, gs_stream *s, gs_gaussians_buffer *gaussians,
                          const gs_gaussian_transform_pod *gaussian_transform,
                          const gs_model_transform_pod *model_transform, const gs_camera *camera,
                          uint32_t band_ty0, uint32_t band_ty1, float *rgba_out_device);

/* Depth and pick planes of a frame (no reference item: the viewer and the editor need them).  Both are
 * full-image H x W row-major planes on the device, like rgba_out_device, and only the band's rows are written.
 *   depth[p] = the sum over the splats pixel p blends of z' * (alpha * T), accumulated in blend order exactly as a colour
 *              channel (D = fma(z', alpha T, D)), z' = the projected view depth (gs_projected.depth); no background term,
 *              so a pixel without contributors holds 0.  The expected depth is depth / rgba.w (the caller divides).
 *   pick[p]  = the CALLER'S index (position in the uploaded buffer) of the first splat, front to back, whose blend step
 *              takes the pixel's transmittance T to <= 1 - pick_threshold (computed in f32), or GS_PICK_NONE.  The step
 *              that finishes a pixel (T (1 - alpha) < 1e-4) is not blended, so it is not picked either.  0.5 picks the
 *              median contributor; any accepted threshold up to 1/255 the first contributor (1 - threshold must
 *              stay below 1 in f32: thresholds of 2^-25 or less are refused).
 * The planes follow the RGBA target: a frame skipped for pair capacity leaves them untouched, and a two-round frame
 * skipped in its second round leaves the first round's state in them (as in the image). */
typedef struct gs_aux_targets {
    float *depth;            /* device, H x W f32 (4-byte aligned), or NULL */
    uint32_t *pick;          /* device, H x W u32 (4-byte aligned), or NULL */
    float pick_threshold;    /* 2^-25 < t < 1; 0.5 = the median contributor */
    uint32_t reserved;       /* 0 */
} gs_aux_targets;
#define GS_PICK_NONE 0xFFFFFFFFu

/* gs_render_frame with the planes of `aux` written by the same blend launch (no extra kernel; the frame makes every other
 * choice as it would without them).  aux == NULL, or both pointers NULL (the threshold is then not looked at): exactly
 * gs_render_frame.  GS_ERR_INVALID_ARGUMENT, before anything is enqueued, for a nonzero `reserved`, and — with a plane —
 * for a threshold outside (0, 1), NaN, or so small that 1 - threshold rounds to 1 in f32 (<= 2^-25), or a misaligned
 * pointer. */
gs_status gs_render_frame_aux(gs_renderer *r, gs_stream *s, gs_gaussians_buffer *gaussians,
                              const gs_gaussian_transform_pod *gaussian_transform,
                              const gs_model_transform_pod *model_transform, const gs_camera *camera,
                              uint32_t band_ty0, uint32_t band_ty1, float *rgba_out_device,
                              const gs_aux_targets *aux);

typedef struct gs_frame_result {
    uint64_t gaussians;       /* N */
    uint64_t visible;         /* V */
    uint64_t pairs;           /* D (the true count, also when it exceeded the capacity) */
    uint64_t pair_capacity;   /* pairs the renderer's buffers hold */
    uint32_t flags;           /* bit 0: pair capacity exceeded; bit 1: the frame was skipped (image not written — but a
                               * two-round frame skipped by its second round leaves the first round's pixel state in
                               * its band: GS_ERR_PAIR_CAPACITY); bit 2: the rank watchdog fired (GS_ERR_RANK_ORDER) */
    uint32_t launches;        /* kernel launches the frame enqueued (after the repack) */
} gs_frame_result;

/* Blocks until the last frame of `r` has completed and reports how it went: GS_OK,
 * GS_ERR_PAIR_CAPACITY (render again), GS_ERR_PAIR_OVERFLOW (> 2^32 pairs) or GS_ERR_HIP.
 * `out` may be NULL. */
gs_status gs_renderer_wait_frame(gs_renderer *r, gs_frame_result *out);

/* How the last frame sorted (blocking like gs_renderer_stats; no reference item: the sorts are the viewer's).  The depth
 * sort runs MSD-first — one scatter on the top 10 bits of the depth key, then one workgroup per bucket finishes the low
 * bits on its CU — while the buckets fit (`bucket_capacity` elements), and as LSD passes while they do not; the renderer
 * chooses per frame from the bucket sizes the previous frames reported.  Both produce the same order. */
typedef struct gs_sort_info {
    uint32_t depth_msd;          /* 1: MSD-first depth sort in the last frame, 0: LSD passes */
    uint32_t depth_bucket_max;   /* largest top-digit bucket the last frame saw (its own report) */
    uint32_t bucket_capacity;    /* elements a bucket may hold for the on-CU path (larger ones take a slow in-kernel fallback) */
    uint32_t tile_msd;           /* the same for the tile sort */
    uint32_t tile_bucket_max;
    uint32_t tile_masks;         /* 1: the last frame dropped unreachable tiles from small rects (tile rect version 4), 0: version 3 */
    uint32_t rounds;             /* rounds the last frame took: 1, or 2 (gs_renderer_set_rounds) */
    uint32_t round1;             /* two rounds: the nearest visible Gaussians its first round covered */
    uint32_t tiles_done;         /* two rounds: tiles the first round finished (every pixel at its final colour) */
    uint32_t partitioned;        /* two rounds: 1 = each round sorted only its own side of a depth threshold */
} gs_sort_info;
gs_status gs_renderer_sort_info(gs_renderer *r, gs_sort_info *out);
/* Pins the choice for the following frames: 1 MSD-first, 0 LSD passes, -1 the renderer chooses (default; the
 * environment variables GS3D_DEPTH_MSD / GS3D_TILE_MSD = 0 / 1 pin it for every renderer of the process).  A pinned
 * MSD-first sort stays correct whatever the bucket sizes (oversized buckets take the in-kernel fallback). */
gs_status gs_renderer_set_sort_mode(gs_renderer *r, int32_t depth_msd, int32_t tile_msd);
/* Tile rect version 4 (no reference item): rects of at most 3 x 3 tiles lose the tiles their splat cannot
 * reach — 5 % fewer (tile, Gaussian) pairs, the same image.  The test costs the preprocess kernel ~120 instructions per
 * Gaussian: hidden where that kernel waits for HBM, a net loss where it does not (50 M x 144 B: +3 %), so by default (-1)
 * it is on for records of 200 bytes or more (f32 SH) in scenes beyond the 256 MiB Infinity Cache; 1 / 0 pin it
 * (GS3D_TILE_MASKS=0/1 pins it for every renderer of the process). */
gs_status gs_renderer_set_tile_masks(gs_renderer *r, int32_t mode);
/* Two-round frames (DESIGN.md 4.2 "rounds"; no reference item: the stages are the viewer's).  A deep scene finishes most
 * of its tiles on the nearest fraction of its Gaussians; the rest is emitted, sorted and staged for nothing.  With two
 * rounds the frame of the nearest `first_round` visible Gaussians (0: a quarter of what the previous frame saw) is
 * rendered first; its blend marks the finished tiles and leaves the pixel state of the others in the image; the second
 * round drops every Gaussian whose rect (at most 3 x 3 tiles) lies in finished tiles and resumes the blend.  The image is
 * the single round's bit for bit; `pairs` of the frame result counts what was emitted (fewer), and the sorted / range
 * taps (gs_renderer_download_sorted, _ranges) refuse such a frame (GS_ERR_INVALID_ARGUMENT).  Each round is bounded by the
 * pairs a round of the previous two-round frame emitted (twice the larger round, with head room; the buffers' capacity
 * without such a report), and a round that outgrows the bound skips the frame (GS_ERR_PAIR_CAPACITY).  Known defect: a
 * frame flagged SKIPPED by its SECOND round has the first round's state in its band of the image — rgb = the first
 * round's colour sums, alpha = a finished pixel's alpha or the raw transmittance, negated once the pixel has stopped
 * (tests/test_gpu_round_bounds.py pins exactly this); skipped by its first round, the image is untouched.  mode: 1 / 0 pin two rounds / one, -1 the renderer chooses
 * (GS3D_ROUNDS=0/1 and GS3D_ROUND1=<count> pin it for every renderer of the process). */
gs_status gs_renderer_set_rounds(gs_renderer *r, int32_t mode, uint32_t first_round);

/* Parity taps on the last frame (blocking).  Sizes: N records / N counts; D keys / D indices;
 * tiles_x*tiles_y*2 ranges. */
gs_status gs_renderer_download_projected(gs_renderer *r, gs_projected *proj_out,
                                         uint32_t *tiles_touched_out, size_t n);
gs_status gs_renderer_download_sorted(gs_renderer *r, uint64_t *keys_out, uint32_t *idx_out,
                                      uint64_t capacity, uint64_t *pairs_out);
gs_status gs_renderer_download_ranges(gs_renderer *r, uint32_t *ranges_out, size_t num_tiles);

/* ------------------------------------------------------------------------------------------ */
/* Gaussian selections (no reference item in the core crate: the reference's      */
/* viewer and editor keep such a bit-per-Gaussian buffer themselves)                             */
/* ------------------------------------------------------------------------------------------ */

/* n bits in device memory, ceil(n / 32) u32 words: bit (i & 31) of word (i >> 5) is Gaussian i in CALLER index order (the
 * position in the uploaded buffer), never mirror order.  Bits at positions >= n of the last word are 0 after every call.
 * Calls that take a stream only ENQUEUE on it unless documented as blocking; using one selection from several streams is
 * the caller's to order, as with any buffer (no reference item). */
typedef struct gs_selection gs_selection;
/* dst = dst op src (no reference item) */
typedef enum { GS_SEL_SET = 0, GS_SEL_OR = 1, GS_SEL_AND = 2, GS_SEL_ANDNOT = 3, GS_SEL_XOR = 4 } gs_select_op;

/* all bits 0 (no reference item) */
gs_status gs_selection_create(gs_device *dev, size_t n, gs_selection **out);
/* (no reference item) */
void gs_selection_destroy(gs_selection *sel);
/* n (no reference item) */
size_t gs_selection_len(const gs_selection *sel);
/* all bits 0 / all n bits 1 / every bit flipped (no reference item) */
gs_status gs_selection_clear(gs_selection *sel, gs_stream *s);
gs_status gs_selection_fill(gs_selection *sel, gs_stream *s);
gs_status gs_selection_invert(gs_selection *sel, gs_stream *s);
/* dst = dst op src; SET copies src, ANDNOT is dst & ~src.  GS_ERR_INVALID_ARGUMENT when the lengths differ (no reference item) */
gs_status gs_selection_combine(gs_selection *dst, gs_stream *s, gs_select_op op, const gs_selection *src);
/* nwords must be ceil(n / 32); bits past n of the uploaded last word are dropped (no reference item) */
gs_status gs_selection_upload(gs_selection *sel, gs_stream *s, const uint32_t *words, size_t nwords);
/* blocking, like the parity taps (no reference item) */
gs_status gs_selection_download(gs_selection *sel, gs_stream *s, uint32_t *words, size_t nwords);
/* number of selected Gaussians: a popcount reduction on the device; blocking (no reference item) */
gs_status gs_selection_count(gs_selection *sel, gs_stream *s, uint64_t *out);

/* sel = sel op {i : |M (p_i, 1) - center|^2 <= radius^2}: pw = M (p, 1) as DESIGN.md 3.2 (sum order ((c0 + c1) + c2) + c3),
 * d = pw - center, (d.x d.x + d.y d.y) + d.z d.z <= radius radius in binary32, every operation rounded, no fma; NaN selects
 * nothing.  Positions are read from the buffer (caller order).  GS_ERR_INVALID_ARGUMENT for a negative or NaN radius or a
 * length mismatch (no reference item) */
gs_status gs_select_sphere(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *gaussians,
                           const gs_model_transform_pod *model_transform, const float center[3], float radius,
                           gs_select_op op);
/* sel = sel op {i : |q.x| <= 1 && |q.y| <= 1 && |q.z| <= 1}, q = B (pw, 1), B = world_to_box, column-major 3 x 4, the same
 * sum order (no reference item) */
gs_status gs_select_box(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *gaussians,
                        const gs_model_transform_pod *model_transform, const float world_to_box[12], gs_select_op op);
/* sel = sel op {i : start <= i < start + count}, word-wise (no reference item).  Only enqueues.  Bits at
 * positions >= n of the last word stay 0 for every op.  After gs_gaussians_buffer_create_concat this is how the pasted part
 * becomes the selection.  GS_ERR_INVALID_ARGUMENT, with the selection unchanged, when start + count > n or the sum overflows. */
gs_status gs_select_range(gs_selection *sel, gs_stream *s, size_t start, size_t count, gs_select_op op);
/* sel = sel op {i : the LAST FRAME of r kept Gaussian i (>= 1 tile: the tiles_touched of gs_renderer_download_projected) and
 * its mean satisfies x0 <= mx < x1, y0 <= my < y1 and — with a plane — mask[floor(my) W + floor(mx)] != 0 (a mean outside
 * the image is then never selected)}.  mask_plane_device: H x W bytes on the device, or NULL.  Gaussians hidden in that
 * frame are not visible.  Enqueued on `s` behind that frame; the renderer's next frame is ordered behind it on any stream;
 * the host does not block.  GS_ERR_INVALID_ARGUMENT without a last frame or on a length mismatch (no reference item) */
gs_status gs_renderer_select_visible(gs_renderer *r, gs_stream *s, gs_selection *sel, float x0, float y0, float x1,
                                     float y1, const uint8_t *mask_plane_device, gs_select_op op);

/* Selections of a frame (no reference item).  hide: its Gaussians are CULLED by the preprocess (all-ones depth
 * key, zero rect; not counted in `visible`, `pairs` or any histogram), so every frame kind — sort modes, list frames, bands,
 * two rounds, aux planes — renders the scene without them.  tint: rgb' = (1 - a) rgb + a t per channel behind the clamp at 0
 * of 3.2 (both products and the sum rounded separately; opacity unchanged), t = tint_rgba[0..2], a = tint_rgba[3].  A
 * Gaussian in both is hidden. */
typedef struct gs_frame_selection {
    const gs_selection *hide;   /* or NULL */
    const gs_selection *tint;   /* or NULL */
    float tint_rgba[4];         /* rgb finite, 0 <= a <= 1 (looked at only with `tint`) */
    uint32_t reserved[2];       /* 0 */
} gs_frame_selection;

/* gs_render_frame_aux with the selections of `fs` (no reference item).  fs == NULL, or both pointers NULL: exactly
 * gs_render_frame_aux — the same bits, kernels and `launches`.  GS_ERR_INVALID_ARGUMENT, before anything is enqueued, for a
 * nonzero `reserved`, a selection whose length differs from the buffer's or that belongs to another device, a non-finite
 * tint or a tint alpha outside [0, 1].  The renderer keeps mirror-slot-ordered copies of the masks and rebuilds one (one
 * launch, counted in `launches`) only when its selection was modified or the buffer's mirror order was rebuilt.  A selection
 * change is no new shape: un-hiding may exceed the pair capacity sized from earlier frames and take the documented skip
 * (GS_ERR_PAIR_CAPACITY, image untouched, the next frame has larger buffers).  (Known defect, not touched here: a two-round
 * frame skipped in its SECOND round leaves part of the first round's state in the image — gs_renderer_set_rounds.) */
gs_status gs_render_frame_sel(gs_renderer *r, gs_stream *s, gs_gaussians_buffer *gaussians,
                              const gs_gaussian_transform_pod *gaussian_transform,
                              const gs_model_transform_pod *model_transform, const gs_camera *camera,
                              uint32_t band_ty0, uint32_t band_ty1, float *rgba_out_device,
                              const gs_aux_targets *aux, const gs_frame_selection *fs);

/* ------------------------------------------------------------------------------------------ */
/* Edits of the selected Gaussians, extraction (no reference item in the core     */
/* crate: the reference's editor moves, recolours and removes Gaussians with compute passes)     */
/* ------------------------------------------------------------------------------------------ */

/* gs_edit.flags; the stages run in this order (no reference item) */
enum { GS_EDIT_TRANSFORM = 1, GS_EDIT_ROTATE_SH = 2, GS_EDIT_COLOR = 4, GS_EDIT_OPACITY = 8 };
/* One edit (no reference item).  Only the fields whose flag is set are looked at. */
typedef struct gs_edit {
    uint32_t flags;
    gs_model_transform_pod transform;  /* pos, rot (xyzw), scale: scale.x == scale.y == scale.z > 0 */
    float color[12];                   /* column-major 3 x 4: rgb' = C (rgb, 1) */
    float opacity[2];                  /* a' = opacity[0] a + opacity[1] */
    uint32_t reserved[4];              /* 0 */
} gs_edit;

/* Applies `e` to every Gaussian of `sel` (NULL: all) in place on the device, for all 12 layouts (DESIGN.md 3.8;
 * no reference item).  Only ENQUEUES on `s` (NULL: the device's internal stream): the next frame of any renderer on any stream is
 * ordered behind it and sees the edited records; downloads and select ops on OTHER streams are the caller's to order, as
 * with any buffer.  A Gaussian outside the selection and a field whose flag is not set keep every byte.  GS_EDIT_ROTATE_SH
 * on an SH-less layout is ignored; flags == 0 launches nothing and dirties nothing.  GS_ERR_INVALID_ARGUMENT, before
 * anything is enqueued, for a null buffer or edit, unknown flag bits, nonzero `reserved`, ROTATE_SH without TRANSFORM, a
 * non-finite field that the flags use, a zero rotation with ROTATE_SH, a scale that is not uniform, not positive or NaN,
 * a selection whose length differs from the buffer's or that belongs to another device. */
gs_status gs_gaussians_buffer_edit(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, const gs_edit *e);
/* New buffer of the same layout (and spatial-order setting) holding the records of `sel` (invert != 0: of its complement;
 * NULL: all / none), caller order kept, bytes unchanged: a stable compaction on the device (DESIGN.md 3.8;
 * no reference item).  Blocking, like gs_selection_count: sizing the new buffer needs the count on the host; *count_out (optional) = its
 * length.  A result of length 0 is what gs_gaussians_buffer_create gives for length 0: GS_OK and a valid buffer whose
 * length is 0 (it owns a 16-byte allocation).  GS_ERR_INVALID_ARGUMENT for a null argument or a selection whose length
 * differs from the buffer's or that belongs to another device; *out is then NULL. */
gs_status gs_gaussians_buffer_create_from_selection(gs_gaussians_buffer *src, gs_stream *s, const gs_selection *sel,
                                                    int32_t invert, gs_gaussians_buffer **out, uint64_t *count_out);
/* Host only: the SH band matrices of a rotation (row-major 3x3, 5x5, 7x7), as the edit uses them: sh'_k = sum_j D[k][j] sh_j
 * per channel and band, defined by sum_k Y_k(d) c'_k = sum_k Y_k(R^T d) c_k for every unit d, R the rotation of the
 * NORMALISED quaternion; computed in double, rounded to binary32 (no reference item).
 * GS_ERR_INVALID_ARGUMENT for a null pointer or a non-finite or zero quaternion. */
gs_status gs_sh_rotation_matrices(const float rot_xyzw[4], float d1[9], float d2[25], float d3[49]);

/* ------------------------------------------------------------------------------------------ */
/* Snapshots of the selected records, concatenation (no reference item in the     */
/* core crate: undo and merging are the reference editor's, done there with whole-buffer copies) */
/* ------------------------------------------------------------------------------------------ */

/* The records of one selection of one buffer, kept on the device with the snapshot's OWN copy of the mask and one u32 per
 * 1024 Gaussians (the first snapshot rank of each block): the undo entry of an edit (no reference item).
 * An inverse edit is no substitute: colour and opacity quantise and clamp, SH re-encodes, rotations are not renormalised. */
typedef struct gs_snapshot gs_snapshot;

/* Captures the records of the Gaussians of `sel` (NULL: all), bytes unchanged, in caller order (DESIGN.md 3.9;
 * no reference item).  BLOCKING, like gs_gaussians_buffer_create_from_selection: the host sizes the allocation from the
 * count.  Ordered behind an edit or restore enqueued on another stream.  The snapshot keeps its own mask: later changes to
 * `sel` do not affect it.  Device memory: count x pod size + 4 ceil(n / 32) + 4 ceil(n / 1024) + 4 bytes, never a
 * whole-buffer copy for a sparse selection.  An empty selection or a buffer of length 0 gives a valid snapshot of count 0.
 * GS_ERR_INVALID_ARGUMENT (*out = NULL) for a null argument or a selection whose length differs from the buffer's or that
 * belongs to another device. */
gs_status gs_gaussians_buffer_snapshot(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, gs_snapshot **out);
/* Frees the snapshot; synchronises the device, so a restore still in flight finishes first (DESIGN.md 3.9;
 * no reference item) */
void gs_snapshot_destroy(gs_snapshot *snap);
/* n of the buffer it was taken from (no reference item) */
size_t gs_snapshot_len(const gs_snapshot *snap);
/* records it holds (no reference item) */
uint64_t gs_snapshot_count(const gs_snapshot *snap);
/* device memory it owns, in bytes (no reference item) */
size_t gs_snapshot_bytes(const gs_snapshot *snap);
/* sel = sel op (the snapshot's mask), so that an undo can also restore what was selected (DESIGN.md 3.9;
 * no reference item).  Only enqueues, like gs_selection_combine.  GS_ERR_INVALID_ARGUMENT when the lengths differ. */
gs_status gs_snapshot_selection(const gs_snapshot *snap, gs_stream *s, gs_selection *sel, gs_select_op op);
/* Writes the snapshot's records back to the indices they came from, in one launch (no reference item).
 * Only ENQUEUES on `s` (NULL: the device's internal stream) and is ordered exactly like gs_gaussians_buffer_edit: behind a
 * mirror rebuild or an earlier edit / restore on another stream; the next frame of any renderer on any stream sees the
 * restored records (the whole mirror is stale, as after a TRANSFORM edit).  A Gaussian outside the snapshot's mask keeps
 * every byte.  The target may be ANY buffer of the same device, layout and length ("paste these records in place");
 * otherwise GS_ERR_INVALID_ARGUMENT before anything is enqueued.  A snapshot of count 0 launches nothing and dirties
 * nothing.  exchange != 0: the same launch swaps — the buffer gets the snapshot's records, the snapshot what the buffer
 * held — so one snapshot is the undo entry and then the redo entry (undo = exchange, redo = exchange again).  The snapshot
 * must stay alive, and must not be used on OTHER streams, until `s` has passed the launch, as with any buffer. */
gs_status gs_gaussians_buffer_restore(gs_gaussians_buffer *g, gs_stream *s, gs_snapshot *snap, int32_t exchange);
/* New buffer holding, for each source in order, the records of sels[i] of srcs[i] (sels == NULL or sels[i] == NULL: all of
 * that source), caller order kept inside each source, bytes unchanged (no reference item).  A source may
 * appear more than once: {g, g} with {NULL, sel} duplicates a selection, {a, b} merges two models (bake a model's transform
 * first with gs_gaussians_buffer_edit).  All sources on one device and of one layout, 1 <= count <= 64, at most 2^32 - 16
 * records in all: otherwise GS_ERR_INVALID_ARGUMENT and *out = NULL.  counts_out (optional, `count` entries) = the records
 * taken per source, so the host knows where each part starts.  BLOCKING, exactly once: the counts of all sources come back
 * in one copy; the copies themselves are only enqueued on `s` (NULL: the device's internal stream) when the call returns.
 * The new buffer is ordered like an edited one (frames, snapshots and extractions on any stream wait for the copies); the
 * sources and selections must not be modified on OTHER streams until `s` has passed the copies.  Ordered behind an edit or
 * restore of a source enqueued on another stream.  The new buffer takes the spatial-order setting of srcs[0]; a total of 0
 * gives the valid length-0 buffer of gs_gaussians_buffer_create. */
gs_status gs_gaussians_buffer_create_concat(gs_stream *s, gs_gaussians_buffer *const *srcs, const gs_selection *const *sels,
                                            uint32_t count, gs_gaussians_buffer **out, uint64_t *counts_out);

/* ------------------------------------------------------------------------------------------ */
/* Attribute statistics, histograms and select by attribute range (no reference  */
/* item in the core crate: the reference's editor computes these on the host from its own copy)  */
/* ------------------------------------------------------------------------------------------ */

/* An attribute maps one record to one binary32 value, the same for all 12 layouts (no reference item).
 * X / Y / Z: pw = M (p, 1), M = model_transform_mat, sum order ((c0 + c1) + c2) + c3 — the arithmetic of gs_select_sphere.
 * RED / GREEN / BLUE / OPACITY: byte j of word 3 divided by 255.  SIZE2: (S00 + S11) + S22 of the layout's decoded 3D
 * covariance, the sum of the squared axis lengths as the renderer sees them (the model transform is not applied).
 * DIST2: d = pw - ref, (d.x d.x + d.y d.y) + d.z d.z.  Every operation is rounded, nothing is fused. */
enum {
    GS_ATTR_X = 0, GS_ATTR_Y = 1, GS_ATTR_Z = 2, GS_ATTR_RED = 3, GS_ATTR_GREEN = 4, GS_ATTR_BLUE = 5,
    GS_ATTR_OPACITY = 6, GS_ATTR_SIZE2 = 7, GS_ATTR_DIST2 = 8, GS_ATTR_COUNT = 9
};
/* One attribute (no reference item).  model_transform == NULL: gs_model_transform_pod_default pushed
 * through the same arithmetic (an infinite coordinate becomes NaN either way). */
typedef struct gs_attribute_desc {
    uint32_t attr;                                   /* GS_ATTR_* */
    const gs_model_transform_pod *model_transform;   /* or NULL */
    float ref[3];                                    /* looked at only for GS_ATTR_DIST2; finite then */
    uint32_t reserved[2];                            /* 0 */
} gs_attribute_desc;

/* One attribute over the selected records (no reference item).  Only finite values enter min, max and
 * sum.  min / max: by the total order on the bit patterns (-0 < +0), so they are bit-defined; +inf / -inf when finite == 0.
 * sum: the values widened to binary64 and added in a fixed shape (no floating-point atomics): the same bits from run to
 * run on the same input; 0 when finite == 0. */
typedef struct gs_attribute_stats {
    uint64_t finite;
    float min, max;
    double sum;
} gs_attribute_stats;
/* count = the selected Gaussians; attr[GS_ATTR_*].  The centroid is sum / finite of X, Y, Z, the bounds their min and max
 * (no reference item). */
typedef struct gs_stats {
    uint64_t count;
    gs_attribute_stats attr[9];
} gs_stats;

/* Statistics of all nine attributes over the records of `sel` (NULL: all) in one pass over the caller-order buffer
 * (no reference item).  BLOCKING, like gs_selection_count.  model_transform == NULL: the default transform;
 * ref == NULL: the origin (ref is GS_ATTR_DIST2's reference point and must be finite).  s == NULL: the device's internal
 * stream.  Ordered behind an edit or restore enqueued on another stream, as gs_gaussians_buffer_snapshot is.  A buffer of
 * length 0 is valid: counts 0, min +inf, max -inf.  The buffer keeps the scratch of the call: calls on ONE buffer from
 * several host threads at once are the caller's to order.  GS_ERR_INVALID_ARGUMENT, before anything is enqueued and with
 * *out untouched, for a null buffer or out, a non-finite ref, a selection whose length differs from the buffer's or that
 * belongs to another device. */
gs_status gs_gaussians_buffer_stats(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel,
                                    const gs_model_transform_pod *model_transform, const float ref[3], gs_stats *out);
/* Histogram of one attribute in one pass (no reference item).  counts_out holds 2 x (bins + 3) values: row 0
 * = the Gaussians of `sel`, row 1 = the others (sel == NULL: everything in row 0).  scale = (float)bins / (hi - lo) in
 * binary32 on the host; the slot of a value v, tested in this order: NaN -> bins + 2; v < lo -> bins; v >= hi -> bins + 1;
 * else (uint32_t)((v - lo) scale), truncated, clamped to bins - 1.  BLOCKING; stream, ordering, scratch and the empty buffer
 * as gs_gaussians_buffer_stats.  GS_ERR_INVALID_ARGUMENT, before anything is enqueued and with counts_out untouched, for a
 * null buffer, descriptor or counts_out, an unknown attribute, nonzero `reserved`, a non-finite ref with GS_ATTR_DIST2,
 * bins outside 1..4096, lo, hi or hi - lo not finite, hi <= lo, a scale that is not finite, a selection whose length
 * differs from the buffer's or that belongs to another device. */
gs_status gs_gaussians_buffer_histogram(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel,
                                        const gs_attribute_desc *a, float lo, float hi, uint32_t bins, uint64_t *counts_out);
/* sel = sel op {i : lo <= v_i && v_i <= hi}, v = the attribute of record i of `gaussians` (DESIGN.md 3.10;
 * no reference item).  Only ENQUEUES; the mask is written word-wise as by gs_select_sphere; ordered behind an edit or restore
 * enqueued on another stream.  A NaN value is never selected, lo > hi selects nothing, infinite bounds are allowed.
 * GS_ATTR_DIST2 with lo = 0, hi = r r is gs_select_sphere(ref, r) bit for bit.  GS_ERR_INVALID_ARGUMENT, before anything is
 * enqueued and with the selection unchanged, for a null argument, an unknown attribute or op, nonzero `reserved`, a
 * non-finite ref with GS_ATTR_DIST2, a NaN bound, a selection whose length differs from the buffer's or that belongs to
 * another device. */
gs_status gs_select_attribute(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *gaussians, const gs_attribute_desc *a,
                              float lo, float hi, gs_select_op op);

/* ------------------------------------------------------------------------------------------ */
/* Neighbour counts and select by neighbourhood (no reference item in the core  */
/* crate: the reference's editor removes floaters on the host from its own copy)                 */
/* ------------------------------------------------------------------------------------------ */

/* The definition (no reference item).  pw_i = M (p_i, 1), the arithmetic of gs_select_sphere and
 * GS_ATTR_X / Y / Z; model_transform == NULL: the default transform through the same arithmetic.  Gaussian i is a POINT iff
 * it belongs to `among` (NULL: all) and the three components of pw_i are finite.  For points i != j, d = pw_i - pw_j: j is a
 * neighbour of i iff (d.x d.x + d.y d.y) + d.z d.z <= r r in binary32, every operation rounded, nothing fused, r r rounded
 * once on the host.  The relation is symmetric; a distance of exactly r counts; r = 0 finds exact duplicates.  c_i = the
 * number of neighbours of i if i is a point, else 0: an integer that does not depend on the traversal, so it is bit-defined.
 *
 * Cost: a 64-bit device sort of n keys (cells of side about r, 21 bits per axis over the bounding box of the points — a far
 * outlier grows the box, not the cells), then for every point the occupancy of the 27 cells around it, cut short by the cap.
 * A radius that puts most of the scene inside one ball, with a large cap, is quadratic by definition: that choice is the
 * caller's.  Both calls only ENQUEUE (the bounding box stays on the device; all 64 key bits are sorted).  The buffer keeps
 * the scratch of the call, 28 bytes per Gaussian, until it is destroyed; a call on another stream waits for the previous one
 * on the device.  Calls on ONE buffer from several host threads at once are the caller's to order. */

/* counts_out[i] = min(c_i, cap), one uint32_t per Gaussian in caller order (no reference item): the input of
 * a density histogram, a heat-map tint or the caller's own threshold; read it back with gs_buffer_download.  counts_out holds
 * at least 4 n bytes on the buffer's device; cap >= 1 (counting for i may stop once it has reached cap).  Only ENQUEUES on `s`
 * (NULL: the device's internal stream), ordered behind an edit or restore enqueued on another stream, as
 * gs_gaussians_buffer_snapshot is.  A buffer of length 0 is valid and launches nothing.  GS_ERR_INVALID_ARGUMENT, before
 * anything is enqueued and with the plane untouched, for a null buffer or plane, a radius that is negative, NaN or infinite or
 * whose square is not finite in binary32, cap == 0, a plane that is too small or on another device, a selection whose length
 * differs from the buffer's or that belongs to another device, a buffer of more than 0xfffffff0 Gaussians. */
gs_status gs_gaussians_buffer_neighbor_counts(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *among,
                                              const gs_model_transform_pod *model_transform, float radius, uint32_t cap,
                                              gs_buffer *counts_out);
/* sel = sel op {i : i is a point and min_count <= c_i <= max_count}, with the true counts (no reference item):
 * max_count = k - 1 selects the floaters with fewer than k others within `radius`.  A Gaussian that is not a point is never
 * selected, not even with min_count = 0; min_count > max_count selects nothing; max_count = UINT32_MAX is "no upper limit".
 * Only ENQUEUES on `s` (NULL: the device's internal stream); the mask is written word-wise as by gs_select_sphere; ordered
 * behind an edit or restore enqueued on another stream.  GS_ERR_INVALID_ARGUMENT, before anything is enqueued and with the
 * selection unchanged, for a null selection or buffer, an unknown op, a radius that is negative, NaN or infinite or whose
 * square is not finite in binary32, a selection (`sel` or `among`) whose length differs from the buffer's or that belongs to
 * another device, a buffer of more than 0xfffffff0 Gaussians. */
gs_status gs_select_neighbors(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *gaussians, const gs_selection *among,
                              const gs_model_transform_pod *model_transform, float radius, uint32_t min_count, uint32_t max_count,
                              gs_select_op op);

/* ------------------------------------------------------------------------------------------ */
/* Layout conversion (no reference item in the core crate: a buffer of the      */
/* reference keeps the layout it was uploaded with)                                             */
/* ------------------------------------------------------------------------------------------ */

/* The definition (no reference item).  convert((S, C) -> (S', C')) maps one record to one record.  Words 0..3
 * (position, colour) are copied.  SH section: S' == S copies its words verbatim, pad included; otherwise each of the 45
 * coefficients is decoded to binary32 as gs_unpack_to_gaussian does (f32: the bits; f16: exact; snorm8: (float)(int8) / 127
 * clamped below at -1; none: +0) and encoded as gs_pack does (f16: round to nearest even; snorm8: truncation, NaN -> 0;
 * none: no words), padding zero.  Cov section: C' == C verbatim; rot-scale -> f32 / f16 is gs_pack's arithmetic; f32 -> f16
 * rounds each of the six words to nearest even; f16 -> f32 is exact; f32 or f16 -> rot-scale is NOT defined
 * (GS_ERR_LOSSY_CONFIG).  Trailing pad words are zero.  Identical layouts keep every byte.  112 of the 144 pairs are defined.
 * For a source that gs_unpack_to_gaussian accepts and pods that gs_pack produced, the result is
 * gs_pack(dst, gs_unpack_to_gaussian(src)) bit for bit. */

/* 1 when records of layout (src_sh, src_cov) convert to (dst_sh, dst_cov), else 0; 0 for an unknown enum value
 * (no reference item) */
int32_t gs_layout_convertible(gs_sh_config src_sh, gs_cov3d_config src_cov, gs_sh_config dst_sh, gs_cov3d_config dst_cov);
/* Host only: converts n records (no reference item); `out` holds n x gs_pod_size(dst_sh, dst_cov) bytes and
 * does not overlap `pods`.  The per-record function is the one the device kernel calls.  GS_ERR_LOSSY_CONFIG for a pair
 * that is not defined, GS_ERR_INVALID_ARGUMENT for a null pointer or an unknown config; `out` is then untouched. */
gs_status gs_convert_pods(gs_sh_config src_sh, gs_cov3d_config src_cov, gs_sh_config dst_sh, gs_cov3d_config dst_cov,
                          const void *pods, size_t n, void *out);
/* New buffer of layout (dst_sh, dst_cov) holding the converted records of `sel` (invert != 0: of its complement; NULL:
 * all / none), caller order kept: the conversion is fused with the stable compaction (no reference item).
 * Blocking, ordered and checked exactly like gs_gaussians_buffer_create_from_selection (behind an edit or restore enqueued
 * on another stream); the result takes the source's spatial-order setting; *count_out (optional) = its length, and a count
 * of 0 gives the valid length-0 buffer of the destination layout.  With identical layouts it IS that call.
 * GS_ERR_LOSSY_CONFIG for a pair that is not defined, before anything is enqueued or allocated; GS_ERR_INVALID_ARGUMENT for
 * a null argument, an unknown config, a selection whose length differs from the buffer's or that belongs to another
 * device; *out is then NULL. */
gs_status gs_gaussians_buffer_create_converted(gs_gaussians_buffer *src, gs_stream *s, const gs_selection *sel, int32_t invert,
                                               gs_sh_config dst_sh, gs_cov3d_config dst_cov, gs_gaussians_buffer **out,
                                               uint64_t *count_out);
/* decompose (no reference item): the six terms xx, yx, zx, yy, zy, zz of one symmetric 3x3 covariance, in
 * the order gs_pack writes them, -> a unit quaternion xyzw with w >= 0 and three scales >= 0 with (R S)(R S)^T = C up to
 * rounding: cyclic Jacobi with a fixed number of sweeps on the matrix prescaled by an even power of two, every operation a
 * rounded binary32 one, the same bits on host and device.  The scales come in Jacobi's column order, unsorted; a diagonal
 * input gives the identity rotation exactly; negative eigenvalues are clamped to 0; an all-zero input gives the identity and
 * +0 scales, a non-finite word the identity and three NaNs (0x7fc00000).  Host only. */
void gs_cov3d_decompose(const float cov[6], float rot_xyzw[4], float scale[3]);
/* Host only: n records of layout (src_sh, src_cov) -> n records of layout (dst_sh, GS_COV3D_ROT_SCALE) (DESIGN.md 3.12a;
 * no reference item).  Words 0..3 and the SH section as gs_convert_pods converts them; the covariance words, decoded to
 * binary32 (f16: exactly), go through gs_cov3d_decompose; trailing pad words are zero.  With src_cov == GS_COV3D_ROT_SCALE it
 * IS gs_convert_pods: all 4 x 3 x 4 combinations are defined.  `out` holds n x gs_pod_size(dst_sh, GS_COV3D_ROT_SCALE) bytes
 * and does not overlap `pods`.  The per-record function is the one the device kernel calls.  GS_ERR_INVALID_ARGUMENT for a
 * null pointer or an unknown config; `out` is then untouched. */
gs_status gs_decompose_pods(gs_sh_config src_sh, gs_cov3d_config src_cov, gs_sh_config dst_sh, const void *pods, size_t n, void *out);
/* New buffer of layout (dst_sh, GS_COV3D_ROT_SCALE) holding the decomposed records (gs_decompose_pods) of `sel`, caller order
 * kept: the decomposition is fused with the stable compaction (no reference item).  Blocking; ordering,
 * argument checks, *count_out, the length-0 result and the spatial-order setting are exactly those of
 * gs_gaussians_buffer_create_converted, and with a rotation + scale source it IS that call.  This is the way from the eight
 * covariance layouts to the exports below and into a rotation + scale scene. */
gs_status gs_gaussians_buffer_create_decomposed(gs_gaussians_buffer *src, gs_stream *s, const gs_selection *sel, int32_t invert,
                                                gs_sh_config dst_sh, gs_gaussians_buffer **out, uint64_t *count_out);
/* gs_gaussians_buffer_create_concat in every respect (1..64 sources on one device, one blocking round trip for the counts,
 * the copies only enqueued, ordering, counts_out, at most 2^32 - 16 records, the spatial-order setting of srcs[0]), but the
 * sources may have ANY layouts: each is converted to (dst_sh, dst_cov), the layout of the new buffer (DESIGN.md 3.12;
 * no reference item).  GS_ERR_LOSSY_CONFIG when a source cannot be converted: nothing is enqueued and *out = NULL. */
gs_status gs_gaussians_buffer_create_concat_as(gs_stream *s, gs_gaussians_buffer *const *srcs, const gs_selection *const *sels,
                                               uint32_t count, gs_sh_config dst_sh, gs_cov3d_config dst_cov,
                                               gs_gaussians_buffer **out, uint64_t *counts_out);

/* ------------------------------------------------------------------------------------------ */
/* Export (no reference item in the core crate: the reference downloads a       */
/* buffer and encodes it on the host)                                                           */
/* ------------------------------------------------------------------------------------------ */

/* The definition (no reference item).  Each call below gives, byte for byte, what the host path gives for the
 * same records: gs_gaussians_buffer_create_from_selection(sel, invert), gs_gaussians_buffer_download_gaussians, then
 * gs_gaussian_to_ply / gs_spz_encode_decompressed / gs_spz_encode / gs_gaussians_write.  Extraction, decoding of the records and
 * encoding run in one kernel on the device; the host receives records that are ready to write.
 * Common to the four calls: `sel` selects the records (invert != 0: its complement; NULL: all / none), caller order kept.
 * Blocking on `s` (NULL: the device's internal stream), ordered behind an edit, restore or concatenation enqueued on another
 * stream.  out == NULL: only the selection is scanned and the count / size is returned (the gzip member of
 * gs_gaussians_buffer_export_spz has to be built to be measured).  GS_ERR_INVALID_ARGUMENT, with `out` untouched, for a null
 * buffer or count pointer, a capacity below the count / size, a selection whose length differs from the buffer's or that
 * belongs to another device.  Only the layouts gs_gaussians_buffer_download_gaussians accepts (SH f32 / f16 / snorm8 with
 * rotation + scale) can be exported; the others return its error, GS_ERR_LOSSY_CONFIG with the reference's message, before
 * anything is enqueued.  A covariance layout with SH is exported through gs_gaussians_buffer_create_decomposed. */

/* Gaussian::to_ply of the selected records on the device (no reference item): *count_out = their number,
 * `out` (capacity in records) receives them.  The source is walked in slices (2 Mi records; GS3D_EXPORT_SLICE=<records, a
 * multiple of 1024> overrides) through two device staging buffers, ordered so that the kernel of one slice can run under the copy of the
 * previous one.  GS_ERR_OUT_OF_MEMORY when the staging buffers cannot be allocated. */
gs_status gs_gaussians_buffer_export_ply(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert,
                                         gs_ply_gaussian_pod *out, size_t capacity, uint64_t *count_out);
/* gs_spz_encode_decompressed of the selected records on the device (no reference item): header and six
 * columns, built in device memory (at most 16 + 65 bytes per record) and copied once.  options == NULL: gs_spz_options_default.
 * capacity and *bytes_out in bytes.  The options are checked as gs_spz_encode_decompressed checks them. */
gs_status gs_gaussians_buffer_export_spz_decompressed(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert,
                                                      const gs_spz_options *options, void *out, size_t capacity, size_t *bytes_out);
/* ... and the gzip member around that payload, as gs_spz_encode writes it (gs_spz_compress: zlib on one host thread)
 * (no reference item) */
gs_status gs_gaussians_buffer_export_spz(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert,
                                         const gs_spz_options *options, void *out, size_t capacity, size_t *bytes_out);
/* The complete file image gs_gaussians_write gives for the selected records (no reference item): for
 * GS_SOURCE_PLY the header of gs_ply_write for their count with the vertices landing directly behind it, for GS_SOURCE_SPZ
 * gs_gaussians_buffer_export_spz with the default options.  GS_SOURCE_INTERNAL fails as gs_gaussians_write does. */
gs_status gs_gaussians_buffer_write(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert,
                                    gs_gaussians_source source, void *out, size_t capacity, size_t *bytes_out);

/* ------------------------------------------------------------------------------------------ */
/* Contribution scores (no reference item in the core crate: pruning and          */
/* compression tools score a Gaussian by what it does to the images of a set of views)           */
/* ------------------------------------------------------------------------------------------ */

/* The definition (no reference item).  A contribution is a pair (pixel, Gaussian) whose blend step at that
 * pixel is taken with alpha_eff > 0 — a step the pick plane would consider.  The step that finishes a pixel
 * (T (1 - alpha) < 1e-4) is not blended and contributes nothing; neither do culled or hidden Gaussians.  Its weight is
 * w = alpha_eff * T, the binary32 product the blend forms; w > 0 always (T >= 1e-4, alpha >= 1/255).  One record per Gaussian
 * in CALLER index order; every field is an integer reduction, so the result does not depend on traversal order, lane
 * grouping, bands or streams: it is defined bit for bit. */
typedef struct gs_contribution {
    uint64_t sum;   /* += (uint32_t)(w * 16777216.0f) per contribution: units of 2^-24, truncated; exact integer adds */
    uint32_t hits;  /* += 1 per contribution (wraps mod 2^32; documented, not checked) */
    float    wmax;  /* max over contributions; all w > 0, so the max of the bit patterns */
} gs_contribution;

/* gs_select_contribution kinds: the value v of a record (no reference item) */
enum {
    GS_CONTRIB_SUM = 0,   /* (float)sum * 0x1p-24f: u64 -> f32 round-to-nearest-even, then the exact scale */
    GS_CONTRIB_HITS = 1,  /* (float)hits */
    GS_CONTRIB_MAX = 2    /* wmax */
};

/* gs_render_frame_sel without aux planes, which also ACCUMULATES the frame's contributions into `contrib`: n records of 16
 * bytes in a caller-owned buffer of at least 16 n bytes (no reference item).  A frame never clears the
 * records: gs_contributions_clear does.  contrib == NULL: exactly gs_render_frame_sel(..., NULL, fs).  With `contrib` the
 * image is bit for bit the plain frame's and so is `launches`: the accumulation rides in the blend launch (the grouped
 * blend, 8x4 blocks where the plain frame would take the ungrouped kernel).  GS_ERR_INVALID_ARGUMENT, before anything is
 * enqueued, for a buffer smaller than 16 n bytes, one that is not 16-byte aligned or one of another device.
 * A contribution frame is planned as ONE round — exactly as a frame under gs_renderer_set_rounds(r, 0, 0), without changing
 * the renderer's pin — because a frame skipped for pair capacity (GS_ERR_PAIR_CAPACITY) must leave the records untouched,
 * always: a two-round frame skipped in its second round could not undo the adds of its first.
 * Frames of several renderers on several streams may accumulate into one buffer concurrently (the adds are atomic); clears
 * and reads are the caller's to order, as with any buffer. */
gs_status gs_render_frame_contrib(gs_renderer *r, gs_stream *s, gs_gaussians_buffer *gaussians,
                                  const gs_gaussian_transform_pod *gaussian_transform,
                                  const gs_model_transform_pod *model_transform, const gs_camera *camera,
                                  uint32_t band_ty0, uint32_t band_ty1, float *rgba_out_device,
                                  const gs_frame_selection *fs, gs_buffer *contrib);
/* Zeroes the first 16 n bytes of `contrib` (no reference item).  Only enqueues on `s`.  GS_ERR_INVALID_ARGUMENT for a null
 * argument, a buffer smaller than 16 n bytes or a stream of another device. */
gs_status gs_contributions_clear(gs_buffer *contrib, gs_stream *s, size_t n);
/* sel = sel op {i : lo <= v_i && v_i <= hi}, v the `kind` value of record i of `contrib` (n = the selection's length;
 * DESIGN.md 3.5c; no reference item).  The argument rules of gs_select_attribute: a NaN bound is refused, lo > hi selects
 * nothing, infinite bounds are allowed; the mask is written word-wise, bits past n stay 0.  Only enqueues.
 * GS_ERR_INVALID_ARGUMENT for an unknown kind or op, a buffer smaller than 16 n bytes, a misaligned one, or objects of
 * different devices. */
gs_status gs_select_contribution(gs_selection *sel, gs_stream *s, gs_buffer *contrib, uint32_t kind, float lo, float hi,
                                 gs_select_op op);

/* ------------------------------------------------------------------------------------------ */
/* Image metrics (no reference item): what a change of the scene did to the    */
/* rendered picture, measured where the pictures are                                            */
/* ------------------------------------------------------------------------------------------ */

/* The definition (no reference item).  Two images of H x W pixels, four binary32 channels r g b a each, in the
 * layout of rgba_out_device.  d_c = a_c - b_c, one binary32 subtraction.  A pixel is FINITE when its eight values are; only
 * finite pixels enter the sums, maxima and `differing`.  The sums are binary64, added in a fixed shape (no floating-point
 * atomics): two calls on the same inputs return the same bytes.
 * SSIM (flag GS_COMPARE_SSIM) is the usual 3DGS metric per colour channel: an 11 x 11 Gaussian window, sigma 1.5, zero padding,
 * every pixel counted.  It is defined operation by operation in binary32, every operation rounded, nothing fused, the
 * division correctly rounded: the weights g[0..10] (binary32 of exp(-(k-5)^2 / 4.5) / sum); the five planes a, b, a a, a b, b b
 * (products rounded per pixel) filtered horizontally, then vertically, each as acc = +0, acc = acc + g[k] v for k = 0..10
 * ascending, samples outside the image +0; C1 = (0.01f L)^2, C2 = (0.03f L)^2; and with ma, mb, eaa, eab, ebb the filtered planes
 *   maa = ma ma, mbb = mb mb, mab = ma mb, saa = eaa - maa, sbb = ebb - mbb, sab = eab - mab,
 *   s = ((2 mab + C1) (2 sab + C2)) / (((maa + mbb) + C1) ((saa + sbb) + C2)).
 * Identical images give s = 1.0f exactly.  A non-finite input makes exactly the windows that contain it non-finite; those
 * values are left out of ssim_sum and ssim_finite.  Against a binary64 evaluation a value is off by about 1e-5 on ordinary
 * images and by up to a few 1e-4 where an image is nearly constant over the window (eaa - maa cancels). */
enum { GS_COMPARE_SSIM = 1 };
/* What gs_image_compare computes besides the error fields (no reference item).  err_plane[p] =
 * fmaxf(fmaxf(fmaxf(|d_r|, |d_g|), |d_b|), |d_a|) of a finite pixel, the quiet NaN 0x7FC00000 of any other;
 * ssim_plane[p] = ((s_r + s_g) + s_b) / 3.0f.  A plane that overlaps an image (or the other plane) is the caller's error. */
typedef struct gs_image_compare_desc {
    uint32_t flags;          /* GS_COMPARE_SSIM or 0 */
    float data_range;        /* L: finite, > 0 (1 for the renderer's images) */
    float *err_plane;        /* device H x W f32, or NULL */
    float *ssim_plane;       /* device H x W f32, or NULL; needs GS_COMPARE_SSIM */
    uint32_t reserved[4];    /* 0 */
} gs_image_compare_desc;
/* The result of gs_image_compare (no reference item).  MSE of channel c = sum_sq[c] / finite; the mean SSIM
 * of channel c = ssim_sum[c] / ssim_finite[c]. */
typedef struct gs_image_metrics {
    uint64_t pixels;         /* W * H */
    uint64_t finite;         /* pixels whose 8 values (4 of a, 4 of b) are all finite */
    uint64_t differing;      /* finite pixels with some d_c != 0 */
    uint64_t bit_differing;  /* pixels (finite or not) where any of the four 32-bit words differs */
    double sum_sq[4];        /* over finite pixels, per channel r g b a: sum of (double)d_c * (double)d_c */
    double sum_abs[4];       /* sum of (double)|d_c| */
    float max_abs[4];        /* max |d_c| over finite pixels; 0 when there is none */
    uint32_t max_abs_at[4];  /* smallest y * W + x that attains it; 0xFFFFFFFF when finite == 0 */
    double ssim_sum[3];      /* r g b: sum of the FINITE per-pixel SSIM values; 0 without the flag */
    uint64_t ssim_finite[3]; /* how many were finite */
} gs_image_metrics;
/* Compares two device images in one pass (no reference item).  `a` and `b` are device pointers to H x W x 4
 * binary32 values, 16-byte aligned; they may be equal.  desc == NULL: flags 0, L = 1, no planes.  BLOCKING, like
 * gs_gaussians_buffer_stats (`out` is host memory); s == NULL: the device's internal stream.  The device keeps the scratch of
 * the call (144 bytes per workgroup, at most 2048 of them); calls on one device from several host threads take
 * turns.  Without GS_COMPARE_SSIM each image is read exactly once.  GS_ERR_INVALID_ARGUMENT, before anything is enqueued and
 * with *out untouched, for a null device, image or out, a zero dimension, W * H > 2^32 - 2, an image that is not 16-byte
 * aligned or a plane that is not 4-byte aligned, unknown flags, nonzero `reserved`, a data_range that is not finite or not
 * positive, ssim_plane without GS_COMPARE_SSIM, a stream of another device. */
gs_status gs_image_compare(gs_device *dev, gs_stream *s, const float *a, const float *b, uint32_t width, uint32_t height,
                           const gs_image_compare_desc *desc, gs_image_metrics *out);

/* ------------------------------------------------------------------------------------------ */
/* Fast gzip members (no reference item): SPZ saved without zlib, the member    */
/* deflated on the device from the payload that is already there                               */
/* ------------------------------------------------------------------------------------------ */

/* The definition (no reference item).  A gzip member (header 1f 8b 08 00 00 00 00 00 00 03, a DEFLATE stream,
 * CRC-32 and length mod 2^32) whose stream holds one block per 32768 input bytes, each starting on a byte boundary: a
 * fixed-Huffman run block for a chunk of >= 4 equal bytes, else a dynamic block of literals only, else a stored block, by the
 * size rule of 3.15; an empty input is the block 03 00.  No string matching: the quantised byte-planar columns of an SPZ
 * payload gain almost nothing from it.  Every inflater reads the member (gs_spz_decompress, zlib, the reference's GzDecoder);
 * it is NOT the bytes gs_spz_compress gives.  The host and the device encoder give the same bytes, whatever the thread count. */

/* The largest member of `len` input bytes: 18 + len + 5 max(1, ceil(len / 32768)) (no reference item) */
size_t gs_gzip_fast_bound(size_t len);
/* The member of `len` host bytes, encoded on the host (no reference item) by up to 32 threads
 * (GS3D_HOST_THREADS overrides).  out == NULL: *bytes_out = its exact size.  GS_ERR_INVALID_ARGUMENT, with nothing written,
 * for a null pointer or a capacity below the size (*bytes_out is still the size). */
gs_status gs_gzip_fast(const void *bytes, size_t len, void *out, size_t capacity, size_t *bytes_out);
/* The member of the `len` DEVICE bytes of `b` from `offset` (any alignment), encoded on the device; `out` is host memory and
 * only the compressed bytes cross the link (no reference item).  Byte-equal to gs_gzip_fast of the same bytes.
 * BLOCKING on `s` (NULL: the device's internal stream).  out == NULL: the exact size (the kernels run, nothing is gathered or
 * copied).  Device memory of the call: 32784 bytes per chunk of 32768 plus the member, freed before it returns.
 * GS_ERR_INVALID_ARGUMENT, with nothing written, for a null buffer or size pointer, a range past the end of the buffer, a
 * capacity below the size, a stream of another device. */
gs_status gs_buffer_gzip_fast(gs_buffer *b, gs_stream *s, size_t offset, size_t len, void *out, size_t capacity, size_t *bytes_out);
/* gs_gaussians_buffer_export_spz with the member of gs_gzip_fast around the same payload (no reference item):
 * the scan and the payload kernel of the export, the payload (16-byte header included) stays on the device and is deflated
 * there.  The arguments, the refused layouts and the errors are those of gs_gaussians_buffer_export_spz; out == NULL returns
 * the exact size.  The member inflates to the bytes of gs_gaussians_buffer_export_spz_decompressed. */
gs_status gs_gaussians_buffer_export_spz_fast(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert,
                                              const gs_spz_options *options, void *out, size_t capacity, size_t *bytes_out);

/* ------------------------------------------------------------------------------------------ */
/* Clusters: connected components within a radius, select by cluster size (DESIGN.md 3.16;     */
/* no reference item): "remove small clusters" and "select all of what I clicked"              */
/* ------------------------------------------------------------------------------------------ */

/* The definition (no reference item).  pw_i, POINT and NEIGHBOUR are those of 3.11 above, unchanged: `among`,
 * the NULL transform, the radius test in binary32 with r r rounded once on the host.  G is the graph on the points whose edges
 * are the neighbour pairs; the relation is symmetric, so its components are well defined.  L_i = the smallest caller index of a
 * point in i's component, GS_COMPONENT_NONE where i is no point.  S_i = the number of points in i's component (a singleton
 * has 1), 0 where i is no point.  All of these are integers that depend on neither the traversal, the grid, the order in which
 * lanes win atomics, nor the run: they are bit-defined.
 *
 * Cost: the sort and the traversal of 3.11 WITHOUT a cap (every candidate pair is visited once), a lock-free union-find over
 * the passing pairs, then one pass per plane.  A radius that puts most of the scene inside one ball is quadratic by
 * definition, as in 3.11; there is no cap and no approximate mode: that choice is the caller's.  The three calls only ENQUEUE.
 * They share the buffer's scratch with the calls of 3.11 and grow it to 44 bytes per Gaussian (28 of 3.11 and four more words:
 * parent, root, smallest index and size per root); a call on another stream waits for the previous user of that scratch on
 * the device.  Calls on ONE buffer from several host threads at once are the caller's to order. */
#define GS_COMPONENT_NONE 0xFFFFFFFFu
typedef struct gs_components_info {
    uint32_t points;         /* the number of points */
    uint32_t components;     /* the number of i with L_i == i */
    uint32_t largest;        /* the maximum of S_i; 0 with no point */
    uint32_t largest_label;  /* the smallest label among the components of that size; GS_COMPONENT_NONE with no point */
} gs_components_info;

/* labels_out[i] = L_i and sizes_out[i] = S_i, one uint32_t per Gaussian in caller order, into device planes of at least 4 n
 * bytes; info_out receives the gs_components_info of the graph, 16 bytes (no reference item).  Each of the
 * three may be NULL, not all of them; bytes behind 4 n (behind 16 for the info) stay as they were.  Read them back with
 * gs_buffer_download.  Only ENQUEUES on `s` (NULL: the device's internal stream), ordered behind an edit or restore enqueued on
 * another stream.  A buffer of length 0 is valid and launches nothing: the info is set to that of a graph without points.
 * GS_ERR_INVALID_ARGUMENT, before anything is enqueued and with planes and info untouched, for a null buffer, three null
 * outputs, a radius that is negative, NaN or infinite or whose square is not finite in binary32, a plane or info buffer that
 * is too small or on another device, a selection whose length differs from the buffer's or that belongs to another device, a
 * buffer of more than 0xfffffff0 Gaussians. */
gs_status gs_gaussians_buffer_components(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *among,
                                         const gs_model_transform_pod *model_transform, float radius, gs_buffer *labels_out,
                                         gs_buffer *sizes_out, gs_buffer *info_out);
/* sel = sel op {i : i is a point and min_size <= S_i <= max_size} (no reference item): max_size = m - 1 selects
 * every cluster smaller than m — the floater clumps a neighbour count cannot see.  A Gaussian that is not a point is never
 * selected, not even with min_size = 0; min_size > max_size selects nothing; max_size = UINT32_MAX is "no upper limit".  Only
 * ENQUEUES on `s` (NULL: the device's internal stream); the mask is written word-wise as by gs_select_sphere, bits at positions
 * >= n stay 0; ordered behind an edit or restore enqueued on another stream; a buffer of length 0 only changes the
 * selection's generation.  GS_ERR_INVALID_ARGUMENT, before anything is enqueued and with the selection unchanged, for a null
 * selection or buffer, an unknown op, a radius that is negative, NaN or infinite or whose square is not finite in binary32, a
 * selection (`sel` or `among`) whose length differs from the buffer's or that belongs to another device, a buffer of more than
 * 0xfffffff0 Gaussians. */
gs_status gs_select_components(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *gaussians, const gs_selection *among,
                               const gs_model_transform_pod *model_transform, float radius, uint32_t min_size, uint32_t max_size,
                               gs_select_op op);
/* sel = sel op {i : i is a point and its component contains a point j with bit j of `seeds` set}
 * (no reference item): a picked index (gs_select_range(idx, 1)) grows to the whole object it belongs to.
 * A seed that is no point seeds nothing; empty seeds select nothing.  `seeds` may be `sel` itself, which grows a selection to whole clusters: the seeds are
 * read completely before `sel` is written.  Enqueueing, ordering, the mask and the errors are those of gs_select_components,
 * with `seeds` (not NULL) checked as `among` is. */
gs_status gs_select_connected(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *gaussians, const gs_selection *among,
                              const gs_model_transform_pod *model_transform, float radius, const gs_selection *seeds,
                              gs_select_op op);

/* ------------------------------------------------------------------------------------------ */
/* Simplify: merge the Gaussians of each grid cell into one (no reference       */
/* item): a preview, a far level of detail, a scene that has to fit a smaller card              */
/* ------------------------------------------------------------------------------------------ */

/* The definition (no reference item).  CELLS are those of 3.11 for radius = cell_size on the STORED positions
 * (no model transform): Gaussian i is a POINT iff it is in `among` (NULL: all) and its three position words are finite; its
 * cell is the 3 x 21-bit key of 3.11, computed in binary64 from the bounding box of the points and
 * h = max(cell_size (1 + 2^-10), extent 2^-21 (1 + 2^-10), 2^-62), so cell membership is bit-defined.  Non-points are dropped.
 * Record k of the result is the k-th occupied cell in ascending key order (z, y, x); K = the number of occupied cells.
 *
 * A cell with ONE member yields that record as gs_convert_pods converts it (gs_decompose_pods where the source is a covariance
 * layout and the destination rotation + scale), bit for bit: an isolated Gaussian stays what it was.
 *
 * A cell with m >= 2 members: every value is decoded to binary32 as gs_unpack_to_gaussian decodes the source layout;
 * alpha_i = byte 3 of word 3 / 255, Sigma_i = the decoded 3D covariance, s_i = (S00 + S11) + S22 (GS_ATTR_SIZE2),
 * w_i = alpha_i s_i; if W = sum w_i is not > 0 or any w_i is not finite, w_i = 1 for the whole cell.  With c = the cell's
 * centre lo + (cell + 0.5) h rounded to binary32 per axis and d_i = p_i - c:
 *   position   c + delta,  delta = sum w_i d_i / W
 *   covariance sum w_i (Sigma_i + d_i d_i^T) / W - delta delta^T, each diagonal term clamped at 0 from below (moments about the
 *              cell centre: the cancellation is bounded by h^2, not by the scene's coordinates)
 *   rgb, each of the 45 SH coefficients   sum w_i x_i / W; a colour byte is trunc(255 x + 0.5), saturated
 *   opacity    clamp(W / ((S00 + S11) + S22), 0, 1) on the merged covariance, 0 if that trace is not > 0; with the w_i = 1
 *              fallback clamp(sum alpha_i / m, 0, 1).  Opacity x size mass is kept: a cell of m identical Gaussians gives back
 *              that Gaussian's position, covariance, colour and SH with the opacity min(1, m alpha).
 * The merged record is the (SH f32, cov f32) record of these values, converted to the destination as gs_convert_pods converts
 * it (a rotation + scale destination: as gs_decompose_pods does, through the device twin of gs_cov3d_decompose).
 * The sums are binary32, added in a fixed shape without floating-point atomics: the same input gives the same bytes on every
 * call, as gs_gaussians_buffer_stats promises for its sums.  THE SHAPE ITSELF IS NOT PART OF THE DEFINITION: a merged cell
 * agrees with a binary64 evaluation of the formulas within (m + 16) 2^-24 sum w_i |t_i| / W per value (t_i: the summed term;
 * a position adds 2^-24 |p| for the rounding of c + delta), not bit for bit. */

/* *out = the simplified buffer of layout (dst_sh, dst_cov) — ALL 12 source and all 12 destination layouts are defined, because
 * a covariance is produced here, not converted — and *count_out (or NULL) = K.  cell_of_out (or NULL): a device plane of at
 * least 4 n bytes; word i receives the output index of the cell Gaussian i went into, 0xffffffff where i is not a point:
 * this is how a caller carries labels, scores or a selection across the merge.  BLOCKING, like
 * gs_gaussians_buffer_create_from_selection: one 4-byte round trip for K.  Ordered behind an edit or restore enqueued on
 * another stream; shares the buffer's scratch with the calls of 3.11 / 3.16 (28 bytes per Gaussian of 3.11, 4 per 256
 * Gaussians for the cell counts, 4 per Gaussian for the cells that are merged again with unit weights, 512 per 64 Gaussians
 * for the sums of cells that cross a wave: 40 bytes per Gaussian) and records its event on every path.  The result takes the source's
 * spatial-order setting; the source is not changed.  n = 0 or K = 0 gives the valid length-0 buffer of the destination layout.
 * GS_ERR_INVALID_ARGUMENT, before anything is enqueued or allocated, with *out = NULL, *count_out = 0 and the plane
 * untouched, for a null src or out, an unknown config, a cell_size that is negative, NaN or infinite or whose square is not
 * finite in binary32, a selection whose length differs from the buffer's or that belongs to another device, a plane that is
 * too small or on another device, a buffer of more than 0xfffffff0 Gaussians. */
gs_status gs_gaussians_buffer_create_simplified(gs_gaussians_buffer *src, gs_stream *s, const gs_selection *among,
                                                float cell_size, gs_sh_config dst_sh, gs_cov3d_config dst_cov,
                                                gs_buffer *cell_of_out /* or NULL */, gs_gaussians_buffer **out,
                                                uint64_t *count_out /* or NULL */);

/* ------------------------------------------------------------------------------------------ */
/* Nearest neighbours: k-NN distances, select by them, their summary (no       */
/* reference item): the radius the calls of 3.11 / 3.16 / 3.17 need, statistical outliers     */
/* ------------------------------------------------------------------------------------------ */

/* The definition (no reference item).  pw_i, POINT, `among`, the NULL transform and the binary32 squared
 * distance d2(i, j) = (d.x d.x + d.y d.y) + d.z d.z, d = pw_i - pw_j, are those of 3.11, unchanged: every operation rounded,
 * nothing fused, rr = r r rounded once on the host.  For a point i, a radius r and 1 <= k <= 16 the CANDIDATES are the points
 * j != i with d2(i, j) <= rr, ordered by the pair (bits of d2, caller index j), smaller first: d2 is never negative and never
 * NaN for points, so the bit order is the value order, and equal distances go to the smaller caller index.  The ROW of i is
 * the first min(k, candidates) of them — k values d2_t ascending and k indices j_t — padded with +inf and GS_KNN_NONE; it is
 * COMPLETE iff there are at least k candidates.  The row depends on neither the traversal, the grid nor the cell size, and a
 * complete row is the same for every larger radius: it is bit-defined, indices included.
 *
 * A STATISTIC maps a row to one binary32 value v.  GS_KNN_KTH_DIST2: v = d2_{k-1}.  GS_KNN_MEAN_DIST: v = s / (float)k with
 * s = ((sqrtf(d2_0) + sqrtf(d2_1)) + ...) + sqrtf(d2_{k-1}), the correctly rounded root and quotient.  Both are +inf for an
 * incomplete row and undefined for a row whose first value is NaN: such a row belongs to no point.
 *
 * Cost: the sort and the traversal of 3.11 without a cap; each point keeps its k best candidates in registers, and its
 * acceptance bound shrinks from rr to its k-th distance once it holds k.  A radius far above the k-th distances costs what
 * the count of 3.11 costs at that radius: quadratic when most of the scene is in one ball. */
#define GS_KNN_NONE 0xFFFFFFFFu
#define GS_KNN_MAX_K 16
enum { GS_KNN_KTH_DIST2 = 0, GS_KNN_MEAN_DIST = 1 };

/* The rows of the Gaussians of `queries` (NULL: all) in caller order, record-major: the row of Gaussian i is dist2_out[i k ..
 * i k + k) (binary32) and index_out[i k .. i k + k) (uint32_t; index_out may be NULL) (no reference item).
 * Each plane holds at least 4 k n bytes on the buffer's device; bytes behind 4 k n and every row outside `queries` keep every
 * byte.  A written row of a Gaussian that is no point (outside `among`, or not finite) is all NaN / GS_KNN_NONE.  Only
 * ENQUEUES on `s` (NULL: the device's internal stream), ordered behind an edit or restore enqueued on another stream; shares
 * the buffer's scratch and its event with the calls of 3.11.  A buffer of length 0 is valid and launches nothing.
 * GS_ERR_INVALID_ARGUMENT, before anything is enqueued and with the planes untouched, for a null buffer or distance plane, a
 * radius that is negative, NaN or infinite or whose square is not finite in binary32, k outside 1..16, a plane that is too
 * small or on another device, a selection (`among` or `queries`) whose length differs from the buffer's or that belongs to
 * another device, a buffer of more than 0xfffffff0 Gaussians. */
gs_status gs_gaussians_buffer_knn(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *among, const gs_selection *queries,
                                  const gs_model_transform_pod *model_transform, uint32_t k, float radius, gs_buffer *dist2_out,
                                  gs_buffer *index_out /* or NULL */);
/* sel = sel op {i : row i is a point's and lo <= v_i <= hi}, v = the statistic `kind` of row i of the plane, computed from the
 * plane alone: n = gs_selection_len(sel) rows of k values (no reference item).  A NaN row is never selected;
 * lo > hi selects nothing; infinite bounds are allowed, and lo = hi = +inf selects exactly the incomplete rows.  Only ENQUEUES
 * on `s` (NULL: the device's internal stream); the mask is written word-wise as by gs_select_sphere.
 * GS_ERR_INVALID_ARGUMENT, before anything is enqueued and with the selection unchanged, for a null selection or plane, an
 * unknown op or kind, k outside 1..16, a NaN bound, a plane that is smaller than 4 k n bytes or on another device. */
gs_status gs_select_knn(gs_selection *sel, gs_stream *s, const gs_buffer *dist2_plane, uint32_t k, uint32_t kind, float lo,
                        float hi, gs_select_op op);
/* What gs_knn_summary fills (no reference item).  points: the rows whose first value is not NaN; complete:
 * those of them that are complete.  min / max of v over the complete rows by the order of the bit patterns, +inf / -inf when
 * there are none; sum and sum_sq of v and v v over the complete rows, widened to binary64 and added in a fixed shape (no
 * floating-point atomics): the same bits from run to run. */
typedef struct gs_knn_summary_result {
    uint64_t points, complete;
    float min, max;
    double sum, sum_sq;
} gs_knn_summary_result;
/* The summary of the statistic `kind` over the n rows of k values of a distance plane (no reference item):
 * mean = sum / complete and variance = sum_sq / complete - mean mean are the caller's, in binary64.  BLOCKING on `s` (NULL:
 * the device's internal stream), like gs_gaussians_buffer_stats.  n = 0 is valid: counts 0, min +inf, max -inf.
 * GS_ERR_INVALID_ARGUMENT, with *out untouched, for a null plane or out, an unknown kind, k outside 1..16, n above 0xfffffff0,
 * a plane smaller than 4 k n bytes. */
gs_status gs_knn_summary(gs_stream *s, const gs_buffer *dist2_plane, uint64_t n, uint32_t k, uint32_t kind,
                         gs_knn_summary_result *out);

/* Stand-alone device primitives used by the frame (also exported for tests and callers):
 * stable LSD radix sort of (u64 key, u32 value) pairs on bits [0, end_bit) — host buffers in/out,
 * blocking; and exclusive prefix sum of u32. */
gs_status gs_sort_pairs_u64(gs_device *dev, gs_stream *s, uint64_t *keys, uint32_t *values,
                            uint64_t count, uint32_t end_bit);
gs_status gs_exclusive_scan_u32(gs_device *dev, gs_stream *s, const uint32_t *in, uint32_t *out,
                                uint64_t count, uint64_t *total_out);

/* ------------------------------------------------------------------------------------------ */
/* Nearest neighbours between two buffers: rows, overlap select, rigid fit (no */
/* reference item): which Gaussians of A have a counterpart in B, how far apart, which transform */
/* ------------------------------------------------------------------------------------------ */

/* The definition (no reference item).  Two buffers, each with its own model transform (NULL: the default pod):
 * pw of a Gaussian of either side is M (p, 1) under ITS transform, in the arithmetic of 3.11; d2(i, j) = (d.x d.x + d.y d.y) +
 * d.z d.z with d = pw_i - pw_j is the binary32 squared distance of 3.11 / 3.18, every operation rounded, nothing fused, rr = r r
 * rounded once on the host.  A TARGET POINT is a Gaussian of the target that belongs to `among` (NULL: all) and whose pw is
 * finite.  A QUERY is a Gaussian of the query buffer that belongs to `queries` (NULL: all); it is a point iff its pw is finite.
 * The CANDIDATES of a query point i are ALL target points j with d2(i, j) <= rr — there is no self-exclusion, the buffers are two
 * — ordered by the pair (bits of d2, target caller index j), smaller first.  The ROW of i is the first min(k, candidates) of
 * them, padded with +inf and GS_KNN_NONE; it is COMPLETE iff there are at least k.  The row depends on neither the traversal,
 * the grid nor the cell size, and a complete row is the same for every larger radius: it is bit-defined, indices included.
 * The planes are those of 3.18, so gs_select_knn and gs_knn_summary take them unchanged, with n = the QUERY buffer's length.
 *
 * The rows of the queries in QUERY caller order, record-major: row i is dist2_out[i k .. i k + k) (binary32) and index_out[i k
 * .. i k + k) (uint32_t TARGET caller indices; index_out may be NULL).  Each plane holds at least 4 k n_q bytes on the buffers'
 * device; bytes behind 4 k n_q and every row outside `queries` keep every byte.  A written row of a query that is no point is
 * all NaN / GS_KNN_NONE; a target without points gives all-incomplete rows.  Only ENQUEUES on `s` (NULL: the device's internal
 * stream), ordered behind an edit or restore of EITHER buffer enqueued on another stream; takes and releases the neighbour
 * scratch and event of BOTH buffers (3.11).  n_q = 0 is valid and launches nothing.
 * GS_ERR_INVALID_ARGUMENT, before anything is enqueued and with the planes untouched, for a null buffer or distance plane,
 * queries_buf == target (that is gs_gaussians_buffer_knn), buffers of different devices, a radius that is negative, NaN or
 * infinite or whose square is not finite in binary32, k outside 1..16, a plane that is too small or on another device, a
 * selection whose length differs from its buffer's or that belongs to another device, either buffer above 0xfffffff0
 * Gaussians. */
gs_status gs_gaussians_buffer_knn_between(gs_gaussians_buffer *queries_buf, gs_gaussians_buffer *target, gs_stream *s,
                                          const gs_selection *queries /* of queries_buf, or NULL */,
                                          const gs_selection *among /* of target, or NULL */,
                                          const gs_model_transform_pod *query_transform /* or NULL */,
                                          const gs_model_transform_pod *target_transform /* or NULL */, uint32_t k, float radius,
                                          gs_buffer *dist2_out, gs_buffer *index_out /* or NULL */);
/* What gs_gaussians_buffer_pair_sums fills (no reference item): 152 bytes.  Query i of `queries` (NULL: all)
 * forms a PAIR with j = index_plane[i k] iff j < len(target) and both pw are finite, so an index at or beyond the target's
 * length (GS_KNN_NONE, or the bytes of a row that was never written) is never dereferenced.  p = pw_i and q = pw_j in binary32
 * as above, then widened.  pairs: their number; sp, sq: the sums of p and q; spq: row-major, spq[3 a + b] = the sum of p_a q_b
 * (exact products); spp, sqq: the sums of (x x + y y) + z z; sdd: the sum of |p - q|^2, computed in binary64 from the widened
 * coordinates the same way.  Every sum is added in the fixed shape of gs_gaussians_buffer_stats (wave, LDS in wave order, one
 * finishing workgroup; no floating-point atomics): the same bits from run to run. */
typedef struct gs_pair_sums {
    uint64_t pairs;
    double sp[3], sq[3], spq[9], spp, sqq, sdd;
} gs_pair_sums;
/* The sums over the pairs that the first column of an index plane of gs_gaussians_buffer_knn_between names (DESIGN.md 3.19;
 * no reference item).  `queries` is the selection given to that call, or a subset of it; the transforms are the ones the pairs are
 * measured under (the caller's to keep equal to the search's).  BLOCKING on `s` (NULL: the device's internal stream), like
 * gs_gaussians_buffer_stats; a query buffer of length 0 gives all zeros.  GS_ERR_INVALID_ARGUMENT, with *out untouched, for a
 * null buffer, plane or out, buffers of different devices, k outside 1..16, a plane smaller than 4 k n_q bytes or on another
 * device, a selection whose length differs from the query buffer's or that belongs to another device, either buffer above
 * 0xfffffff0 Gaussians. */
gs_status gs_gaussians_buffer_pair_sums(gs_gaussians_buffer *queries_buf, gs_gaussians_buffer *target, gs_stream *s,
                                        const gs_selection *queries /* or NULL */,
                                        const gs_model_transform_pod *query_transform /* or NULL */,
                                        const gs_model_transform_pod *target_transform /* or NULL */, const gs_buffer *index_plane,
                                        uint32_t k, gs_pair_sums *out);
/* The similarity transform `delta` that brings the p of the pairs onto their q in the least-squares sense, from the sums alone:
 * host, binary64, no device (no reference item).  Horn's closed form: centroids, H = spq - sp sq^T / pairs, the
 * largest eigenvector of the symmetric 4 x 4 matrix of H by cyclic Jacobi with a fixed count of 12 sweeps, the quaternion
 * normalised to w >= 0; scale 1, or with_scale != 0 the least-squares uniform scale; t = mean q - s R mean p.  *rms_out (may be
 * NULL) = sqrt(sdd / pairs), the RMS distance of the pairs as they came in.  delta acts in world space AFTER the query's
 * transform: composed with it (below) it is the query transform of the next search.  GS_ERR_INVALID_ARGUMENT, with the
 * outputs untouched, for a null sums or delta_out, fewer than 3 pairs, a sum that is not finite, p without spread, a rotation
 * the pairs do not determine (collinear p or q: the two largest eigenvalues closer than 2^-40 of the matrix norm), a scale
 * that is not positive. */
gs_status gs_rigid_fit(const gs_pair_sums *sums, int32_t with_scale, gs_model_transform_pod *delta_out, double *rms_out /* or NULL */);
/* out = the pod of delta o m for a delta of uniform scale s_d = delta->scale[0] (no reference item): rot = r_d r
 * (quaternion product), scale = s_d scale, pos = s_d R_d pos + t_d, in binary64, rounded once; exact as a matrix product even
 * when m scales non-uniformly, because the scale of a pod acts before its rotation.  out may be delta or m; a null argument
 * does nothing. */
void gs_model_transform_compose(const gs_model_transform_pod *delta, const gs_model_transform_pod *m, gs_model_transform_pod *out);

#ifdef __cplusplus
}
#endif
#endif /* GS3D_H */
