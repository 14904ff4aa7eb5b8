// gs_core.hip — the part of the C ABI of include/gs3d.h every other unit rests on: errors and environment switches, the
// POD helpers, devices / streams / buffers / downloads, Gaussian buffers with their device load paths (pack, PLY, SPZ)
// and the transform buffers.  Kernels: gs_pack_kernels.h.
#include "gs_host.h"

#include <cstdarg>
#include <thread>

#include "gs_pack_kernels.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------

static thread_local gs_error_info t_err = {0, 0, 0, 0, {0}};

gs_status gs_fail(gs_status code, uint64_t a, uint64_t b, uint64_t c, const char *fmt, ...) {
    t_err.code = code;
    t_err.a = a;
    t_err.b = b;
    t_err.c = c;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err.message, sizeof(t_err.message), fmt, ap);
    va_end(ap);
    return code;
}

// ------------------------------------------------------------------------------------------------
// environment switches (gsp::Switches, gs_policy.h): read once, on the first use of any of them
// ------------------------------------------------------------------------------------------------

static bool env_on(const char *name) {      // NAME=1 switches on
    const char *e = std::getenv(name);
    return e && e[0] == '1';
}
static bool env_off(const char *name) {     // NAME=0 switches off
    const char *e = std::getenv(name);
    return e && e[0] == '0';
}
static long env_int(const char *name, long dflt) {
    const char *e = std::getenv(name);
    return e ? std::atol(e) : dflt;
}
// the three variables that are read again at every call (parallel_for, gs_device_create, buffer creation)
static const char *env_now(const char *name) { return std::getenv(name); }

static gsp::Switches read_switches() {
    gsp::Switches s;
    s.roctx = env_on("GS3D_ROCTX");
    s.event_fence = env_on("GS3D_EVENT_FENCE");
    s.frame_event = env_on("GS3D_FRAME_EVENT");
    s.test_rank_fault = env_on("GS3D_TEST_RANK_FAULT");
    if (const char *e = std::getenv("GS3D_TEST_RANK_WATCH")) {
        s.test_rank_watch_set = true;
        s.test_rank_watch = (uint32_t)std::strtoul(e, nullptr, 10);
    }
    s.rect_v1 = env_on("GS3D_RECT_V1");
    s.rect32_off = env_off("GS3D_RECT32");
    s.wt_stores = (int)env_int("GS3D_WT_STORES", s.wt_stores);
    s.wt_records = (int)env_int("GS3D_WT_RECORDS", s.wt_records);
    s.scan_rows_small_off = env_off("GS3D_SCAN_ROWS_SMALL");
    s.nt_scatter = (int)env_int("GS3D_NT_SCATTER", s.nt_scatter);
    s.chunk_hist_off = env_off("GS3D_CHUNK_HIST");
    s.narrow_keys_off = env_off("GS3D_NARROW_KEYS");
    s.xcd_remap_off = env_off("GS3D_XCD_REMAP");
    s.xcd_remap_c = (int)env_int("GS3D_XCD_REMAP_C", s.xcd_remap_c);
    s.depth_sort_large = (int)env_int("GS3D_DEPTH_SORT_LARGE", s.depth_sort_large);
    s.tile_sort_large = (int)env_int("GS3D_TILE_SORT_LARGE", s.tile_sort_large);
    s.tile_masks = (int)env_int("GS3D_TILE_MASKS", s.tile_masks);
    s.depth_msd = (int)env_int("GS3D_DEPTH_MSD", s.depth_msd);
    s.blend_groups = (int)env_int("GS3D_BLEND_GROUPS", s.blend_groups);
    s.blend_free_body = (int)env_int("GS3D_BLEND_FREE_BODY", s.blend_free_body);
    s.rounds = (int)env_int("GS3D_ROUNDS", s.rounds);
    s.round1 = env_int("GS3D_ROUND1", s.round1);
    s.round_partition = (int)env_int("GS3D_ROUND_PARTITION", s.round_partition);
    s.force_banded = (int)env_int("GS3D_FORCE_BANDED", s.force_banded);
    s.mask_rec = (int)env_int("GS3D_MASK_REC", s.mask_rec);
    s.nt_loads = (int)env_int("GS3D_NT_LOADS", s.nt_loads);
    s.block_cull_off = env_off("GS3D_BLOCK_CULL");
    s.block_list = (int)env_int("GS3D_BLOCK_LIST", s.block_list);
    s.pre_serial = env_off("GS3D_PRE_PIPELINE");
    s.cursor_kernel = (int)env_int("GS3D_CURSOR_KERNEL", s.cursor_kernel);
    s.expand_xcd = (int)env_int("GS3D_EXPAND_XCD", s.expand_xcd);
    s.tile_msd = (int)env_int("GS3D_TILE_MSD", s.tile_msd);
    s.tile_msd_auto = env_on("GS3D_TILE_MSD_AUTO");
    s.ranges_in_blend = (int)env_int("GS3D_RANGES_IN_BLEND", s.ranges_in_blend);
    s.ranges_search = (int)env_int("GS3D_RANGES_SEARCH", s.ranges_search);
    s.export_slice = env_int("GS3D_EXPORT_SLICE", s.export_slice);
    return s;
}

const gsp::Switches &gsh::switches() {
    static const gsp::Switches s = read_switches();
    return s;
}

extern "C" void gs_last_error(gs_error_info *out) {
    if (out) *out = t_err;
}

extern "C" uint32_t gs_abi_version(void) { return GS3D_ABI_VERSION; }

extern "C" void gs_hip_versions(int32_t *compiled, int32_t *runtime, int32_t *driver) {
    if (compiled) *compiled = HIP_VERSION;
    int v = 0;
    if (runtime) *runtime = hipRuntimeGetVersion(&v) == hipSuccess ? v : 0;
    v = 0;
    if (driver) *driver = hipDriverGetVersion(&v) == hipSuccess ? v : 0;
}

extern "C" const char *gs_status_string(gs_status s) {
    switch (s) {
    case GS_OK: return "ok";
    case GS_ERR_INVALID_ARGUMENT: return "invalid argument";
    case GS_ERR_NO_DEVICE: return "no HIP device";
    case GS_ERR_HIP: return "HIP runtime error";
    case GS_ERR_OUT_OF_MEMORY: return "out of device memory";
    case GS_ERR_COUNT_MISMATCH: return "Gaussians count mismatch";
    case GS_ERR_RANGE_COUNT_MISMATCH: return "Gaussians range count mismatch";
    case GS_ERR_BUFFER_SIZE_NOT_MULTIPLE: return "buffer size and expected multiple size mismatch";
    case GS_ERR_BUFFER_SIZE_MISMATCHED: return "buffer size and expected size mismatch";
    case GS_ERR_RESOURCE_COUNT_MISMATCH: return "resource count and bind group layout count mismatch";
    case GS_ERR_WORKGROUP_SIZE_EXCEEDS_LIMIT: return "workgroup size exceeds device limit";
    case GS_ERR_MISSING_BIND_GROUP_LAYOUT: return "missing bind group layout for compute bundle";
    case GS_ERR_MISSING_RESOLVER: return "missing resolver for compute bundle";
    case GS_ERR_MISSING_ENTRY_POINT: return "missing entry point for compute bundle";
    case GS_ERR_MISSING_MAIN_SHADER: return "missing main shader for compute bundle";
    case GS_ERR_KERNEL_COMPILE: return "kernel compilation failed";
    case GS_ERR_LOSSY_CONFIG: return "configuration cannot be converted back to a Gaussian";
    case GS_ERR_DOWNLOAD: return "buffer download failed";
    case GS_ERR_PAIR_OVERFLOW: return "more than 2^32 (tile, Gaussian) pairs";
    case GS_ERR_PAIR_CAPACITY: return "pair capacity exceeded; render again";
    case GS_ERR_RANK_ORDER: return "radix rank watchdog fired; device switched to the ballot-based rank; render again";
    case GS_ERR_PLY: return "PLY read error";
    case GS_ERR_SPZ: return "SPZ read error";
    default: return "unknown";
    }
}

// ------------------------------------------------------------------------------------------------
// host-side data model: packing (G::from_gaussian) — runs on the host in the reference too
// ------------------------------------------------------------------------------------------------

extern "C" size_t gs_pod_size(gs_sh_config sh, gs_cov3d_config cov) {
    if (!valid_cfg(sh, cov)) return 0;
    return (size_t)gs::pod_bytes(sh, cov);
}

static const char *k_feature_names[7] = {"sh_single", "sh_half", "sh_norm8", "sh_none",
                                         "cov3d_rot_scale", "cov3d_single", "cov3d_half"};

extern "C" const char *gs_feature_name(uint32_t index) {
    return index < 7 ? k_feature_names[index] : nullptr;
}

extern "C" gs_status gs_pod_features(gs_sh_config sh, gs_cov3d_config cov, uint8_t out[7]) {
    if (!valid_cfg(sh, cov) || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bad config");
    for (int i = 0; i < 7; i++) out[i] = (i == (int)sh) || (i == 4 + (int)cov);
    return GS_OK;
}

template <class F>
static void parallel_for(size_t n, F fn) {
    unsigned hw = std::thread::hardware_concurrency();
    size_t threads = n < 65536 ? 1 : (hw ? (hw > 32 ? 32 : hw) : 4);
    if (const char *e = env_now("GS3D_HOST_THREADS")) threads = std::atoi(e) > 0 ? (size_t)std::atoi(e) : threads;
    if (threads <= 1) {
        fn((size_t)0, n);
        return;
    }
    std::vector<std::thread> pool;
    size_t per = (n + threads - 1) / threads;
    for (size_t t = 0; t < threads; t++) {
        size_t a = t * per, b = a + per < n ? a + per : n;
        if (a >= b) break;
        pool.emplace_back([=] { fn(a, b); });
    }
    for (auto &th : pool) th.join();
}

// G::from_gaussian on the host: the same encoders the device kernel uses (gs_pack_kernels.h)
static void pack_one(int sh, int cov, const gs_gaussian &g, uint8_t *p, size_t stride) {
    static_assert(sizeof(gs_gaussian) == gs::GAUSSIAN_WORDS * 4, "gs_gaussian layout");
    uint32_t gw[gs::GAUSSIAN_WORDS], pw[56];
    std::memcpy(gw, &g, sizeof(gw));
    gs::pack_words(sh, cov, gw, pw);
    std::memcpy(p, pw, stride);
}

extern "C" gs_status gs_pack(gs_sh_config sh, gs_cov3d_config cov, const gs_gaussian *in, size_t n,
                             void *out) {
    if (!valid_cfg(sh, cov) || (n && (!in || !out)))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "gs_pack: bad argument");
    size_t stride = gs_pod_size(sh, cov);
    uint8_t *o = (uint8_t *)out;
    parallel_for(n, [=](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) pack_one(sh, cov, in[i], o + i * stride, stride);
    });
    return GS_OK;
}

extern "C" gs_status gs_unpack_to_gaussian(gs_sh_config sh, gs_cov3d_config cov, const void *pods,
                                           size_t n, gs_gaussian *out) {
    if (!valid_cfg(sh, cov) || (n && (!pods || !out)))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "gs_unpack_to_gaussian: bad argument");
    if (sh == GS_SH_NONE)
        return gs_fail(GS_ERR_LOSSY_CONFIG, 0, 0, 0, "Cannot convert from SH None configuration");
    if (cov == GS_COV3D_SINGLE)
        return gs_fail(GS_ERR_LOSSY_CONFIG, 0, 0, 0, "Cannot convert from Cov3d Single configuration");
    if (cov == GS_COV3D_HALF)
        return gs_fail(GS_ERR_LOSSY_CONFIG, 0, 0, 0, "Cannot convert from Cov3d Half configuration");
    size_t stride = gs_pod_size(sh, cov);
    const uint8_t *in = (const uint8_t *)pods;
    parallel_for(n, [=](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            uint32_t pw[56], gw[gs::GAUSSIAN_WORDS];
            std::memcpy(pw, in + i * stride, stride);
            gs::unpack_words(sh, pw, gw);       // the same code the device kernel runs (k_unpack_pods)
            std::memcpy(&out[i], gw, sizeof(gw));
        }
    });
    return GS_OK;
}

extern "C" gs_status gs_max_std_dev_encode(float v, uint8_t *out) {
    if (!out || !(v >= 0.0f && v <= 3.0f))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "max_std_dev must be in [0, 3]");
    *out = (uint8_t)(v / 3.0f * 255.0f);
    return GS_OK;
}

extern "C" float gs_max_std_dev_decode(uint8_t v) { return (float)v / 255.0f * 3.0f; }

extern "C" gs_status gs_gaussian_transform_pod_new(float size, gs_display_mode mode, uint8_t sh_deg,
                                                   uint8_t no_sh0, float max_std_dev,
                                                   gs_gaussian_transform_pod *out) {
    if (!out || (int)mode < 0 || (int)mode > 2)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bad display mode");
    if (sh_deg > 3) return gs_fail(GS_ERR_INVALID_ARGUMENT, sh_deg, 0, 0, "SH degree must be in [0, 3]");
    uint8_t sd;
    GS_TRY(gs_max_std_dev_encode(max_std_dev, &sd));
    out->size = size;
    out->flags[0] = (uint8_t)mode;
    out->flags[1] = sh_deg;
    out->flags[2] = no_sh0 ? 1 : 0;
    out->flags[3] = sd;
    return GS_OK;
}

extern "C" void gs_gaussian_transform_pod_default(gs_gaussian_transform_pod *out) {
    gs_gaussian_transform_pod_new(1.0f, GS_DISPLAY_SPLAT, 3, 0, 3.0f, out);
}

extern "C" void gs_model_transform_pod_new(const float pos[3], const float rot[4],
                                           const float scale[3], gs_model_transform_pod *out) {
    std::memset(out, 0, sizeof(*out));
    std::memcpy(out->pos, pos, 12);
    std::memcpy(out->rot, rot, 16);
    std::memcpy(out->scale, scale, 12);
}

extern "C" void gs_model_transform_pod_default(gs_model_transform_pod *out) {
    const float p[3] = {0, 0, 0}, r[4] = {0, 0, 0, 1}, s[3] = {1, 1, 1};
    gs_model_transform_pod_new(p, r, s, out);
}

// ------------------------------------------------------------------------------------------------
// device / stream / buffer
// ------------------------------------------------------------------------------------------------

gs_status gsh::use_device(const gs_device *dev) {
    if (!dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null device");
    GS_HIP(hipSetDevice(dev->ordinal));
    // HIP's "last error" is sticky per thread: drop whatever an earlier, already reported failure
    // left behind so that the hipGetLastError() checks after our launches only see our launches
    (void)hipGetLastError();
    return GS_OK;
}

extern "C" gs_status gs_device_create(int32_t ordinal, gs_device **out) {
    if (!out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null out");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return gs_fail(GS_ERR_NO_DEVICE, (uint64_t)e, 0, 0, "no HIP device available (%s)",
                    e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (ordinal < 0 || ordinal >= count)
        return gs_fail(GS_ERR_NO_DEVICE, 0, 0, 0, "device ordinal %d out of range [0, %d)", ordinal, count);
    GS_HIP(hipSetDevice(ordinal));
    hipDeviceProp_t props;
    GS_HIP(hipGetDeviceProperties(&props, ordinal));
    gs_device *d = new gs_device();
    d->ordinal = ordinal;
    d->limits.max_compute_workgroup_size_x = (uint32_t)props.maxThreadsDim[0];
    d->limits.max_compute_invocations_per_workgroup = (uint32_t)props.maxThreadsPerBlock;
    d->limits.compute_units = (uint32_t)props.multiProcessorCount;
    d->limits.wavefront_size = (uint32_t)props.warpSize;
    d->limits.total_memory_bytes = (uint64_t)props.totalGlobalMem;
    std::snprintf(d->limits.arch_name, sizeof(d->limits.arch_name), "%s", props.gcnArchName);
    hipError_t se = d->internal.create();
    if (se != hipSuccess) {
        delete d;
        return gs_fail(GS_ERR_HIP, (uint64_t)se, 0, 0, "hipStreamCreate failed: %s", hipGetErrorString(se));
    }
    // the LDS-atomic ordering the fast radix ranking relies on
    d->lds_atomic_ordered = !env_now("GS3D_DISABLE_FAST_RANK") && probe_lds_atomic_order(d->internal.s);
    *out = d;
    return GS_OK;
}

extern "C" int32_t gs_device_fast_rank(const gs_device *dev) { return dev && dev->lds_atomic_ordered.load() ? 1 : 0; }

extern "C" void gs_device_destroy(gs_device *dev) {
    if (!dev) return;
    (void)hipSetDevice(dev->ordinal);
    delete dev;
}

extern "C" gs_status gs_device_limits(const gs_device *dev, gs_limits *out) {
    if (!dev || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    *out = dev->limits;
    return GS_OK;
}

extern "C" gs_status gs_device_synchronize(gs_device *dev) {
    GS_TRY(use_device(dev));
    GS_HIP(hipDeviceSynchronize());
    return GS_OK;
}

extern "C" gs_status gs_stream_create(gs_device *dev, gs_stream **out) {
    if (!out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null out");
    GS_TRY(use_device(dev));
    hipStream_t s;
    GS_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = new gs_stream(dev, s, true);
    return GS_OK;
}

extern "C" gs_status gs_device_stream_priority_range(gs_device *dev, int32_t *least, int32_t *greatest) {
    GS_TRY(use_device(dev));
    int lo = 0, hi = 0;
    GS_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    if (least) *least = lo;
    if (greatest) *greatest = hi;
    return GS_OK;
}

extern "C" gs_status gs_stream_create_with_priority(gs_device *dev, int32_t priority, gs_stream **out) {
    if (!out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null out");
    GS_TRY(use_device(dev));
    int lo = 0, hi = 0;
    GS_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    if (priority > lo || priority < hi)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)(int64_t)priority, 0, 0, "stream priority %d outside [%d (least), %d (greatest)]",
                    priority, lo, hi);
    hipStream_t s;
    GS_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority));
    *out = new gs_stream(dev, s, true);
    return GS_OK;
}

extern "C" gs_status gs_stream_wrap(gs_device *dev, void *hip_stream, gs_stream **out) {
    if (!dev || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    *out = new gs_stream(dev, (hipStream_t)hip_stream, false);
    return GS_OK;
}

extern "C" void *gs_stream_native(const gs_stream *s) { return s ? (void *)s->s : nullptr; }

extern "C" gs_status gs_stream_synchronize(gs_stream *s) {
    if (!s) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null stream");
    GS_TRY(use_device(s->dev));
    GS_HIP(hipStreamSynchronize(s->s));
    return GS_OK;
}

extern "C" void gs_stream_destroy(gs_stream *s) {
    if (!s) return;
    // A renderer whose last frame was enqueued on this stream records its end-of-frame event lazily, on the stream, when
    // it moves elsewhere (gs_render_frame): do that now, while the handle is alive.  This holds for wrapped streams too
    // (gs_stream_wrap): destroy the gs_stream BEFORE the hipStream_t it wraps.
    (void)hipSetDevice(s->dev->ordinal);
    renderers_leave_stream(s->dev, s->s);
    delete s;
}

gs_buffer *gsh::make_buffer(gs_device *dev, void *ptr, size_t bytes, bool owned) {
    return new gs_buffer{dev, ptr, bytes, owned};
}

extern "C" gs_status gs_buffer_create(gs_device *dev, size_t bytes, const void *init,
                                      gs_buffer **out) {
    if (!out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null out");
    GS_TRY(use_device(dev));
    DevMem p;
    // a zero-sized wgpu buffer is legal; keep a 16-byte allocation so the pointer is valid
    GS_HIP_AS("hipMalloc(&p, bytes ? bytes : 16)", p.alloc_raw(bytes ? bytes : 16));
    if (init && bytes) {
        hipError_t e = hipMemcpy(p.ptr, init, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "hipMemcpy failed: %s", hipGetErrorString(e));
    } else if (bytes) {
        // wgpu zero-initialises new buffers.  hipMemset of device memory runs on the null stream and may return before it
        // has run; the caller's streams are non-blocking and do not wait for that stream, so the fill is awaited here —
        // or it may land on top of what the caller writes next
        hipError_t e = hipMemset(p.ptr, 0, bytes);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "hipMemset failed: %s", hipGetErrorString(e));
    }
    *out = make_buffer(dev, p.release(), bytes, true);
    return GS_OK;
}

extern "C" gs_status gs_buffer_from_raw(gs_device *dev, void *device_ptr, size_t bytes,
                                        gs_buffer **out) {
    if (!dev || !out || (!device_ptr && bytes))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    *out = make_buffer(dev, device_ptr, bytes, false);
    return GS_OK;
}

extern "C" gs_buffer *gs_buffer_retain(gs_buffer *b) {
    if (b) b->refs.fetch_add(1);
    return b;
}

extern "C" void gs_buffer_release(gs_buffer *b) {
    if (!b) return;
    if (b->refs.fetch_sub(1) == 1) {
        if (b->owned && b->ptr) {
            (void)hipSetDevice(b->dev->ordinal);
            (void)hipFree(b->ptr);
        }
        delete b;
    }
}

extern "C" size_t gs_buffer_size(const gs_buffer *b) { return b ? b->bytes : 0; }
extern "C" void *gs_buffer_device_ptr(const gs_buffer *b) { return b ? b->ptr : nullptr; }

extern "C" gs_status gs_buffer_write(gs_buffer *b, gs_stream *s, size_t offset, const void *src,
                                     size_t bytes) {
    if (!b || (bytes && !src)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (offset > b->bytes || bytes > b->bytes - offset)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, offset, bytes, b->bytes,
                    "write of %zu bytes at offset %zu overruns buffer of %zu bytes", bytes, offset,
                    b->bytes);
    if (!bytes) return GS_OK;
    GS_TRY(use_device(b->dev));
    hipStream_t st = stream_of(b->dev, s);
    GS_HIP(hipMemcpyAsync((uint8_t *)b->ptr + offset, src, bytes, hipMemcpyHostToDevice, st));
    // queue.write_buffer captures `src` at call time: do not return while the host memory may
    // still be read by an in-flight staged copy.
    GS_HIP(hipStreamSynchronize(st));
    return GS_OK;
}

hipError_t gsh::fetch(hipStream_t st, void *dst, const void *src, size_t bytes) {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
}

extern "C" gs_status gs_buffer_download(gs_buffer *b, gs_stream *s, void *dst, size_t bytes) {
    if (!b || (bytes && !dst)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (bytes > b->bytes)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, bytes, b->bytes, 0,
                    "download of %zu bytes from buffer of %zu bytes", bytes, b->bytes);
    if (!bytes) return GS_OK;
    GS_TRY(use_device(b->dev));
    const hipError_t e = fetch(stream_of(b->dev, s), dst, b->ptr, bytes);
    if (e != hipSuccess)
        return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    return GS_OK;
}

// BufferWrapper::prepare_download / map_download (src/buffer/mod.rs:48-101): the copy into a
// host-visible staging buffer is only ENQUEUED; the caller maps (waits for) it later.
struct gs_download {
    gs_device *dev = nullptr;
    size_t bytes = 0;
    Event done;
    Pinned<void> pinned;
};

extern "C" gs_status gs_buffer_prepare_download(gs_buffer *b, gs_stream *s, gs_download **out) {
    if (!b || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    *out = nullptr;
    GS_TRY(use_device(b->dev));
    std::unique_ptr<gs_download> d(new gs_download());
    d->dev = b->dev;
    d->bytes = b->bytes;
    hipError_t e = d->pinned.alloc(b->bytes ? b->bytes : 1, hipHostMallocDefault);
    if (e == hipSuccess) e = d->done.create();
    hipStream_t st = stream_of(b->dev, s);
    if (e == hipSuccess && b->bytes) e = hipMemcpyAsync(d->pinned.ptr, b->ptr, b->bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(d->done, st);
    if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    *out = d.release();
    return GS_OK;
}

extern "C" int32_t gs_download_ready(gs_download *d) {
    if (!d) return 0;
    (void)hipSetDevice(d->dev->ordinal);
    const hipError_t e = hipEventQuery(d->done);
    (void)hipGetLastError();
    return e == hipSuccess ? 1 : 0;
}

extern "C" gs_status gs_download_map(gs_download *d, const void **data_out, size_t *bytes_out) {
    if (!d || !data_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(use_device(d->dev));
    const hipError_t e = hipEventSynchronize(d->done);
    if (e != hipSuccess)
        return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    *data_out = d->pinned.ptr;
    if (bytes_out) *bytes_out = d->bytes;
    return GS_OK;
}

extern "C" void gs_download_release(gs_download *d) {
    if (!d) return;
    (void)hipSetDevice(d->dev->ordinal);
    (void)hipEventSynchronize(d->done);     // the copy may still be writing the staging memory
    delete d;
}

// ------------------------------------------------------------------------------------------------
// GaussiansBuffer<G>
// ------------------------------------------------------------------------------------------------

gs_status gsh::dev_reserve(DevArray &a, size_t bytes) {
    if (a.bytes >= bytes && a.ptr) return GS_OK;
    if (a.ptr) GS_HIP(hipFree(a.ptr));
    a.ptr = nullptr;
    a.bytes = 0;
    size_t want = bytes + bytes / 8 + 256;
    GS_HIP(hipMalloc(&a.ptr, want));
    a.bytes = want;
    return GS_OK;
}

gs_status gsh::dev_alloc(void **out, size_t bytes, uint64_t b, const char *what) {
    *out = nullptr;
    const hipError_t e = hipMalloc(out, bytes);
    if (e == hipSuccess) return GS_OK;
    *out = nullptr;
    return gs_fail(e == hipErrorOutOfMemory ? GS_ERR_OUT_OF_MEMORY : GS_ERR_HIP, (uint64_t)e, b, 0, "%s failed: %s", what, hipGetErrorString(e));
}

gs_status gsh::wait_for_edits(const gs_gaussians_buffer *g, hipStream_t st) {
    if (g->edit_done && st != g->edit_stream) GS_HIP(hipStreamWaitEvent(st, g->edit_done, 0));
    return GS_OK;
}

gs_status gsh::record_edit(gs_gaussians_buffer *g, hipStream_t st) {
    if (!g->edit_done) GS_HIP_AS("hipEventCreateWithFlags(&g->edit_done, hipEventDisableTiming)", g->edit_done.create());
    GS_HIP(hipEventRecord(g->edit_done, st));
    g->edit_stream = st;
    return GS_OK;
}

gs_status gsh::records_check(const gs_gaussians_buffer *g, const gs_stream *s, const gs_selection *sel, int32_t invert, RecordsAccess &a) {
    GS_TRY(check_buffer_selection(g, s, sel));
    a.len = gs_gaussians_buffer_len(g);
    GS_TRY(check_len32(a.len));
    a.dev = g->buf->dev;
    a.n = (uint32_t)a.len;
    a.nblocks = (a.n + gs::PLANAR_BLOCK - 1u) / gs::PLANAR_BLOCK;
    a.words = sel ? sel->bits() : nullptr;
    a.inv = invert ? 1u : 0u;
    return GS_OK;
}

gs_status gsh::records_access(const gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert, RecordsAccess &a) {
    GS_TRY(records_check(g, s, sel, invert, a));
    GS_TRY(use_device(a.dev));
    a.st = stream_of(a.dev, s);
    return wait_for_edits(g, a.st);
}

uint64_t gsh::next_object_id() {
    static std::atomic<uint64_t> next{0};
    return ++next;
}

extern "C" size_t gs_gaussians_buffer_len(const gs_gaussians_buffer *g) {
    return g ? g->buf->bytes / pod_stride(g) : 0;
}

extern "C" gs_status gs_gaussians_buffer_from_buffer(gs_buffer *buffer, gs_sh_config sh,
                                                     gs_cov3d_config cov,
                                                     gs_gaussians_buffer **out) {
    if (!buffer || !out || !valid_cfg(sh, cov))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bad argument");
    size_t stride = gs_pod_size(sh, cov);
    // the kernels move records as 16-byte vectors: an adopted raw pointer (gs_buffer_from_raw) must
    // be 16-byte aligned, as every hipMalloc allocation is
    if ((uintptr_t)buffer->ptr & 15u)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)(uintptr_t)buffer->ptr, 16, 0,
                    "Gaussian buffer device pointer must be 16-byte aligned");
    if (buffer->bytes % stride != 0)
        return gs_fail(GS_ERR_BUFFER_SIZE_NOT_MULTIPLE, buffer->bytes, stride, 0,
                    "buffer size and expected multiple size mismatch: %zu %% %zu != 0",
                    buffer->bytes, stride);
    gs_gaussians_buffer *g = new gs_gaussians_buffer();
    g->buf = gs_buffer_retain(buffer);
    g->sh = sh;
    g->cov = cov;
    {   // default: spatial order on; GS3D_SPATIAL_ORDER=0 keeps the mirror in index order
        const char *e = env_now("GS3D_SPATIAL_ORDER");
        g->spatial = !(e && e[0] == '0');
    }
    *out = g;
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_create(gs_device *dev, gs_sh_config sh, gs_cov3d_config cov,
                                                const void *pods, size_t len,
                                                gs_gaussians_buffer **out) {
    if (!out || !valid_cfg(sh, cov)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bad argument");
    gs_buffer *b = nullptr;
    GS_TRY(gs_buffer_create(dev, len * gs_pod_size(sh, cov), pods, &b));
    gs_status st = gs_gaussians_buffer_from_buffer(b, sh, cov, out);
    gs_buffer_release(b);
    return st;
}

typedef void (*pack_fn)(const uint32_t *, uint64_t, uint32_t *);
static pack_fn k_tbl_pack[4][3] = GS_CFG_TABLE(gs::k_pack_pods);

extern "C" gs_status gs_pack_device(gs_device *dev, gs_stream *s, gs_sh_config sh, gs_cov3d_config cov,
                                    const gs_gaussian *gaussians_device, size_t n, void *pods_device) {
    if (!dev || !valid_cfg(sh, cov) || (n && (!gaussians_device || !pods_device)))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "gs_pack_device: bad argument");
    if (((uintptr_t)gaussians_device | (uintptr_t)pods_device) & 3u)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "gs_pack_device: pointers must be 4-byte aligned");
    GS_TRY(use_device(dev));
    if (!n) return GS_OK;
    const uint64_t groups = ((uint64_t)n + gs::PACK_GROUP - 1) / gs::PACK_GROUP;
    if (groups > 0x7fffffffull) return gs_fail(GS_ERR_INVALID_ARGUMENT, n, 0, 0, "too many Gaussians");
    hipLaunchKernelGGL(k_tbl_pack[sh][cov], dim3((uint32_t)groups), dim3(256), 0, stream_of(dev, s),
                       (const uint32_t *)gaussians_device, (uint64_t)n, (uint32_t *)pods_device);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

static pack_fn k_tbl_from_ply[4][3] = GS_CFG_TABLE(gs::k_from_ply_pods);

extern "C" gs_status gs_pack_device_from_ply(gs_device *dev, gs_stream *s, gs_sh_config sh, gs_cov3d_config cov,
                                             const gs_ply_gaussian_pod *ply_device, size_t n, void *pods_device) {
    if (!dev || !valid_cfg(sh, cov) || (n && (!ply_device || !pods_device)))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "gs_pack_device_from_ply: bad argument");
    if (((uintptr_t)ply_device | (uintptr_t)pods_device) & 3u)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "gs_pack_device_from_ply: pointers must be 4-byte aligned");
    GS_TRY(use_device(dev));
    if (!n) return GS_OK;
    const uint64_t groups = ((uint64_t)n + gs::PACK_GROUP - 1) / gs::PACK_GROUP;
    if (groups > 0x7fffffffull) return gs_fail(GS_ERR_INVALID_ARGUMENT, n, 0, 0, "too many Gaussians");
    hipLaunchKernelGGL(k_tbl_from_ply[sh][cov], dim3((uint32_t)groups), dim3(256), 0, stream_of(dev, s),
                       (const uint32_t *)ply_device, (uint64_t)n, (uint32_t *)pods_device);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// Source records on the host (struct Gaussian, or PlyGaussianPod when `from_ply`) -> PODs in `g` at
// [start, start + count): the records cross PCIe as they are, slice by slice through TWO staging
// buffers (the host stages and submits slice i + 1 while the kernel of slice i runs; copies and kernels
// share one stream, so the transfers themselves run one after the other — the link is the bound:
// 49.7 GB/s of PLY bytes at 50 M vertices), and are converted on the device.
// The caller's memory may be reused when this returns.
static gs_status upload_records(gs_gaussians_buffer *g, gs_stream *s, size_t start, const void *records, size_t count,
                                bool from_ply) {
    constexpr size_t PACK_SLICE = 2u << 20;     // 2 Mi records: 2 x 496 MiB of staging at most
    gs_device *dev = g->buf->dev;
    GS_TRY(use_device(dev));
    if (!count) return GS_OK;
    hipStream_t st = stream_of(dev, s);
    const size_t rec = from_ply ? sizeof(gs_ply_gaussian_pod) : sizeof(gs_gaussian);
    const size_t slice = count < PACK_SLICE ? count : PACK_SLICE;
    const int nbuf = count > slice ? 2 : 1;
    DevMem staging[2];
    Event used[2];
    // (no early return: the stream is synchronised before anything is freed, as it always was, also when the second
    // allocation fails)
    gs_status rc = GS_OK;
    for (int i = 0; i < nbuf && rc == GS_OK; i++) {
        hipError_t e = staging[i].alloc_raw(slice * rec);
        if (e != hipSuccess) rc = gs_fail(GS_ERR_OUT_OF_MEMORY, slice * rec, 0, 0, "hipMalloc failed: %s", hipGetErrorString(e));
        else if ((e = used[i].create()) != hipSuccess)
            rc = gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "hipEventCreate failed: %s", hipGetErrorString(e));
    }
    const size_t stride = pod_stride(g);
    int k = 0;
    for (size_t first = 0; first < count && rc == GS_OK; first += slice, k ^= (nbuf - 1)) {
        const size_t cnt = count - first < slice ? count - first : slice;
        // the staging buffer's previous kernel must have read it before the next copy overwrites it
        if (first >= (size_t)nbuf * slice && hipEventSynchronize(used[k].e) != hipSuccess) {
            rc = gs_fail(GS_ERR_HIP, 0, 0, 0, "upload failed");
            break;
        }
        hipError_t e = hipMemcpyAsync(staging[k].ptr, (const uint8_t *)records + first * rec, cnt * rec, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) {
            rc = gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "upload failed: %s", hipGetErrorString(e));
            break;
        }
        void *dst = (uint8_t *)g->buf->ptr + (start + first) * stride;
        rc = from_ply ? gs_pack_device_from_ply(dev, s, (gs_sh_config)g->sh, (gs_cov3d_config)g->cov,
                                                (const gs_ply_gaussian_pod *)staging[k].ptr, cnt, dst)
                      : gs_pack_device(dev, s, (gs_sh_config)g->sh, (gs_cov3d_config)g->cov, (const gs_gaussian *)staging[k].ptr,
                                       cnt, dst);
        if (rc == GS_OK && hipEventRecord(used[k].e, st) != hipSuccess) rc = gs_fail(GS_ERR_HIP, 0, 0, 0, "upload failed");
    }
    // the staging buffers are freed at the return and the caller's memory may be reused: wait for everything
    if (hipStreamSynchronize(st) != hipSuccess && rc == GS_OK) rc = gs_fail(GS_ERR_HIP, 0, 0, 0, "pack failed");
    return rc;
}

static gs_status upload_gaussians(gs_gaussians_buffer *g, gs_stream *s, size_t start, const gs_gaussian *gaussians,
                                  size_t count) {
    return upload_records(g, s, start, gaussians, count, false);
}

extern "C" gs_status gs_gaussians_buffer_create_from_ply(gs_device *dev, gs_sh_config sh, gs_cov3d_config cov,
                                                         const gs_ply_gaussian_pod *ply, size_t len,
                                                         gs_gaussians_buffer **out) {
    if (!valid_cfg(sh, cov) || (len && !ply) || !out)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bad argument");
    GS_TRY(gs_gaussians_buffer_create(dev, sh, cov, nullptr, len, out));
    gs_status rc = upload_records(*out, nullptr, 0, ply, len, true);
    if (rc != GS_OK) {
        gs_gaussians_buffer_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

// SPZ: the decompressed payload crosses PCIe once; one kernel decodes the columns (Gaussian::from_spz,
// src/gaussian.rs:134-229) and packs (G::from_gaussian)
typedef void (*spz_fn)(gs::SpzView, uint64_t, uint32_t *);
static spz_fn k_tbl_from_spz[4][3] = GS_CFG_TABLE(gs::k_from_spz_pods);

// the n > 0 records of a checked payload -> dst, on the device's own stream; blocks
static gs_status decode_spz_payload(gs_device *dev, const void *bytes, const gs_spz_header &h, const size_t off[6], uint32_t ncoef,
                                    gs_gaussians_buffer *dst) {
    const size_t n = h.num_points;
    const size_t used = off[5] + n * 3u * ncoef;             // the payload the header declares (len may be larger)
    DevMem staging;
    hipError_t e = staging.alloc_raw(used);
    if (e != hipSuccess) return gs_fail(GS_ERR_OUT_OF_MEMORY, used, 0, 0, "hipMalloc failed: %s", hipGetErrorString(e));
    if ((e = hipMemcpyAsync(staging.ptr, bytes, used, hipMemcpyHostToDevice, dev->internal.s)) != hipSuccess)
        return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "upload failed: %s", hipGetErrorString(e));
    const uint8_t *b = (const uint8_t *)staging.ptr;
    gs::SpzView v{b + off[0], b + off[1], b + off[2], b + off[3], b + off[4], b + off[5], h.version, h.fractional_bits, ncoef};
    const uint64_t groups = ((uint64_t)n + gs::PACK_GROUP - 1) / gs::PACK_GROUP;
    hipLaunchKernelGGL(k_tbl_from_spz[dst->sh][dst->cov], dim3((uint32_t)groups), dim3(256), 0, dev->internal.s, v, (uint64_t)n,
                       (uint32_t *)dst->buf->ptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(dev->internal.s);      // (the staging memory is freed at the return)
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "SPZ decode kernel failed: %s", hipGetErrorString(e));
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_create_from_spz_decompressed(gs_device *dev, gs_sh_config sh,
                                                                      gs_cov3d_config cov, const void *bytes,
                                                                      size_t len, gs_spz_header *header_out,
                                                                      gs_gaussians_buffer **out) {
    if (!valid_cfg(sh, cov) || !bytes || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bad argument");
    *out = nullptr;
    gs_spz_header h;
    size_t off[6];
    uint32_t ncoef = 0;
    GS_TRY(gs_spz_payload_layout(bytes, len, &h, off, &ncoef));
    if (header_out) *header_out = h;
    GS_TRY(gs_gaussians_buffer_create(dev, sh, cov, nullptr, h.num_points, out));
    if (!h.num_points) return GS_OK;
    const gs_status rc = decode_spz_payload(dev, bytes, h, off, ncoef, *out);
    if (rc != GS_OK) {
        gs_gaussians_buffer_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

extern "C" gs_status gs_gaussians_buffer_create_from_spz(gs_device *dev, gs_sh_config sh, gs_cov3d_config cov,
                                                         const void *bytes, size_t len, gs_spz_header *header_out,
                                                         gs_gaussians_buffer **out) {
    if (!bytes || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bad argument");
    std::vector<uint8_t> raw;
    GS_TRY(gs_spz_gunzip(bytes, len, raw));
    return gs_gaussians_buffer_create_from_spz_decompressed(dev, sh, cov, raw.data(), raw.size(), header_out, out);
}

extern "C" gs_status gs_gaussians_buffer_update_range_ply(gs_gaussians_buffer *g, gs_stream *s, size_t start,
                                                          const gs_ply_gaussian_pod *ply, size_t count) {
    if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null buffer");
    size_t len = gs_gaussians_buffer_len(g);
    if (count > len || start > len - count)
        return gs_fail(GS_ERR_RANGE_COUNT_MISMATCH, count, start, len,
                    "Gaussians count mismatch: %zu + %zu > %zu", count, start, len);
    if (count && !ply) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null ply records");
    g->mark(start, start + count);
    return upload_records(g, s, start, ply, count, true);
}

extern "C" gs_status gs_gaussians_buffer_create_from_gaussians(gs_device *dev, gs_sh_config sh,
                                                               gs_cov3d_config cov,
                                                               const gs_gaussian *gaussians,
                                                               size_t len,
                                                               gs_gaussians_buffer **out) {
    if (!valid_cfg(sh, cov) || (len && !gaussians) || !out)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bad argument");
    GS_TRY(gs_gaussians_buffer_create(dev, sh, cov, nullptr, len, out));
    gs_status rc = upload_gaussians(*out, nullptr, 0, gaussians, len);
    if (rc != GS_OK) {
        gs_gaussians_buffer_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

extern "C" void gs_gaussians_buffer_destroy(gs_gaussians_buffer *g) {
    if (!g) return;
    (void)hipSetDevice(g->buf->dev->ordinal);
    delete g;
}

extern "C" gs_buffer *gs_gaussians_buffer_buffer(const gs_gaussians_buffer *g) {
    return g ? g->buf : nullptr;
}
extern "C" gs_sh_config gs_gaussians_buffer_sh(const gs_gaussians_buffer *g) {
    return (gs_sh_config)(g ? g->sh : 0);
}
extern "C" gs_cov3d_config gs_gaussians_buffer_cov3d(const gs_gaussians_buffer *g) {
    return (gs_cov3d_config)(g ? g->cov : 0);
}

extern "C" gs_status gs_gaussians_buffer_update(gs_gaussians_buffer *g, gs_stream *s,
                                                const void *pods, size_t count) {
    if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null buffer");
    size_t len = gs_gaussians_buffer_len(g);
    if (count != len)
        return gs_fail(GS_ERR_COUNT_MISMATCH, count, len, 0, "Gaussians count mismatch: %zu != %zu",
                    count, len);
    g->mark_all();
    return gs_buffer_write(g->buf, s, 0, pods, count * pod_stride(g));
}

extern "C" gs_status gs_gaussians_buffer_update_range(gs_gaussians_buffer *g, gs_stream *s,
                                                      size_t start, const void *pods,
                                                      size_t count) {
    if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null buffer");
    size_t len = gs_gaussians_buffer_len(g);
    if (count > len || start > len - count)      // (start + count could wrap)
        return gs_fail(GS_ERR_RANGE_COUNT_MISMATCH, count, start, len,
                    "Gaussians count mismatch: %zu + %zu > %zu", count, start, len);
    g->mark(start, start + count);
    return gs_buffer_write(g->buf, s, start * pod_stride(g), pods, count * pod_stride(g));
}

extern "C" gs_status gs_gaussians_buffer_update_gaussians(gs_gaussians_buffer *g, gs_stream *s,
                                                          const gs_gaussian *gaussians,
                                                          size_t count) {
    if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null buffer");
    size_t len = gs_gaussians_buffer_len(g);
    if (count != len)
        return gs_fail(GS_ERR_COUNT_MISMATCH, count, len, 0, "Gaussians count mismatch: %zu != %zu",
                    count, len);
    if (count && !gaussians) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null gaussians");
    g->mark_all();
    return upload_gaussians(g, s, 0, gaussians, count);
}

extern "C" gs_status gs_gaussians_buffer_update_range_gaussians(gs_gaussians_buffer *g, gs_stream *s,
                                                                size_t start,
                                                                const gs_gaussian *gaussians,
                                                                size_t count) {
    if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null buffer");
    size_t len = gs_gaussians_buffer_len(g);
    if (count > len || start > len - count)
        return gs_fail(GS_ERR_RANGE_COUNT_MISMATCH, count, start, len,
                    "Gaussians count mismatch: %zu + %zu > %zu", count, start, len);
    if (count && !gaussians) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null gaussians");
    g->mark(start, start + count);
    return upload_gaussians(g, s, start, gaussians, count);
}

extern "C" gs_status gs_gaussians_buffer_download(gs_gaussians_buffer *g, gs_stream *s,
                                                  void *pods_out, size_t count) {
    if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null buffer");
    if (count > gs_gaussians_buffer_len(g))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, count, gs_gaussians_buffer_len(g), 0, "count too large");
    return gs_buffer_download(g->buf, s, pods_out, count * pod_stride(g));
}

// GaussiansBuffer::download::<Gaussian> (src/buffer/gaussian.rs:186-196): the PODs are converted back
// on the DEVICE (k_unpack_pods, slice by slice through a staging buffer) and the struct Gaussian
// records come over PCIe ready to use; bit-equal to downloading the PODs and gs_unpack_to_gaussian.
typedef void (*unpack_fn)(const uint32_t *, uint64_t, uint32_t *);
static unpack_fn k_tbl_unpack[3] = {gs::k_unpack_pods<0>, gs::k_unpack_pods<1>, gs::k_unpack_pods<2>};

extern "C" gs_status gs_gaussians_buffer_download_gaussians(gs_gaussians_buffer *g, gs_stream *s,
                                                            gs_gaussian *out, size_t count) {
    if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null buffer");
    if (g->sh == GS_SH_NONE || g->cov != GS_COV3D_ROT_SCALE)
        return gs_unpack_to_gaussian((gs_sh_config)g->sh, (gs_cov3d_config)g->cov, out, 0, out);   // the reference's error
    if (count > gs_gaussians_buffer_len(g))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, count, gs_gaussians_buffer_len(g), 0, "count too large");
    if (!count) return GS_OK;
    if (!out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null out");
    gs_device *dev = g->buf->dev;
    GS_TRY(use_device(dev));
    hipStream_t st = stream_of(dev, s);
    constexpr size_t SLICE = 2u << 20;
    const size_t slice = count < SLICE ? count : SLICE;
    DevMem staging;
    hipError_t e = staging.alloc_raw(slice * sizeof(gs_gaussian));
    if (e != hipSuccess)
        return gs_fail(GS_ERR_OUT_OF_MEMORY, slice * sizeof(gs_gaussian), 0, 0, "hipMalloc failed: %s", hipGetErrorString(e));
    const size_t stride = pod_stride(g);
    for (size_t first = 0; first < count; first += slice) {
        const size_t cnt = count - first < slice ? count - first : slice;
        const uint64_t groups = ((uint64_t)cnt + gs::PACK_GROUP - 1) / gs::PACK_GROUP;
        hipLaunchKernelGGL(k_tbl_unpack[g->sh], dim3((uint32_t)groups), dim3(256), 0, st,
                           (const uint32_t *)((const uint8_t *)g->buf->ptr + first * stride), (uint64_t)cnt, (uint32_t *)staging.ptr);
        e = hipGetLastError();
        // every slice is awaited before the next one, and the last one before the staging memory is freed at the return
        if (e == hipSuccess) e = fetch(st, out + first, staging.ptr, cnt * sizeof(gs_gaussian));
        if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    }
    return GS_OK;
}

extern "C" void gs_gaussians_buffer_mark_dirty(gs_gaussians_buffer *g) {
    if (g) g->mark_all();
}

// ------------------------------------------------------------------------------------------------
// fixed-size uniform buffers
// ------------------------------------------------------------------------------------------------

static gs_status fixed_from_buffer(gs_buffer *b, size_t expected) {
    if (!b) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null buffer");
    if (b->bytes != expected)
        return gs_fail(GS_ERR_BUFFER_SIZE_MISMATCHED, b->bytes, expected, 0,
                    "buffer size and expected size mismatch: %zu != %zu", b->bytes, expected);
    return GS_OK;
}

extern "C" gs_status gs_gaussian_transform_buffer_create(gs_device *dev, gs_buffer **out) {
    gs_gaussian_transform_pod pod;
    gs_gaussian_transform_pod_default(&pod);
    return gs_buffer_create(dev, sizeof(pod), &pod, out);
}
extern "C" gs_status gs_gaussian_transform_buffer_update(gs_buffer *b, gs_stream *s,
                                                         const gs_gaussian_transform_pod *pod) {
    GS_TRY(fixed_from_buffer(b, sizeof(*pod)));
    return gs_buffer_write(b, s, 0, pod, sizeof(*pod));
}
extern "C" gs_status gs_gaussian_transform_buffer_from_buffer(gs_buffer *b) {
    return fixed_from_buffer(b, sizeof(gs_gaussian_transform_pod));
}
extern "C" gs_status gs_model_transform_buffer_create(gs_device *dev, gs_buffer **out) {
    gs_model_transform_pod pod;
    gs_model_transform_pod_default(&pod);
    return gs_buffer_create(dev, sizeof(pod), &pod, out);
}
extern "C" gs_status gs_model_transform_buffer_update(gs_buffer *b, gs_stream *s,
                                                      const gs_model_transform_pod *pod) {
    GS_TRY(fixed_from_buffer(b, sizeof(*pod)));
    return gs_buffer_write(b, s, 0, pod, sizeof(*pod));
}
extern "C" gs_status gs_model_transform_buffer_from_buffer(gs_buffer *b) {
    return fixed_from_buffer(b, sizeof(gs_model_transform_pod));
}
