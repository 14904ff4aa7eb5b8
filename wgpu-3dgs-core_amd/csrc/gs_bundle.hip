// gs_bundle.hip — ComputeBundle: the built-in kernels of gs_bundle_kernels.h and kernels compiled from source with hiprtc
// against gs_kernel_lib.h (the virtual header <wgpu_3dgs_core.h>).
#include "gs_host.h"

#include <hip/hiprtc.h>

#include <string>

#include "gs_bundle_kernels.h"
#include "_gen_kernel_lib_src.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// ComputeBundle
// ------------------------------------------------------------------------------------------------

typedef void (*bundle_kernel_fn)(gs::BundleArgs, uint32_t);

static bundle_kernel_fn k_tbl_test_gaussian[4][3] = GS_CFG_TABLE(gs::k_test_gaussian);
static bundle_kernel_fn k_tbl_unpack_soa[4][3] = GS_CFG_TABLE(gs::k_unpack_soa);

static void release_group(std::vector<gs_buffer *> &g) {
    for (gs_buffer *x : g) gs_buffer_release(x);
    g.clear();
}

struct gs_bundle : NoCopy {
    ~gs_bundle() {
        for (auto &g : groups) release_group(g);
        if (module) {
            (void)hipSetDevice(dev->ordinal);
            (void)hipModuleUnload(module);
        }
    }
    gs_device *dev = nullptr;
    std::string label;
    gs_kernel_id kernel = GS_KERNEL_COUNT_;
    int sh = 0, cov = 0;
    uint32_t workgroup_size = 0;
    std::vector<uint32_t> layout;                     // bindings per group
    std::vector<std::vector<gs_buffer *>> groups;     // managed bind groups (retained)
    bool managed = false;
    bool has_additional_constant = false;
    uint32_t additional_constant = 0;
    uint32_t last_workgroups = 0;
    // bundles compiled from source (gs_bundle_create_from_source)
    bool from_source = false;
    hipModule_t module = nullptr;
    hipFunction_t func = nullptr;
};

extern "C" gs_status gs_bundle_create(gs_device *dev, const gs_bundle_desc *desc, gs_bundle **out) {
    if (!dev || !desc || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if ((int)desc->kernel < 0 || desc->kernel >= GS_KERNEL_COUNT_ || !valid_cfg(desc->sh, desc->cov))
        return gs_fail(GS_ERR_MISSING_MAIN_SHADER, 0, 0, 0, "unknown kernel id %d", (int)desc->kernel);
    if (desc->bind_group_count == 0 || !desc->bindings_per_group)
        return gs_fail(GS_ERR_MISSING_BIND_GROUP_LAYOUT, 0, 0, 0,
                    "missing bind group layout for compute bundle");
    // compute_bundle.rs:269-281
    uint32_t limit = dev->limits.max_compute_workgroup_size_x <
                             dev->limits.max_compute_invocations_per_workgroup
                         ? dev->limits.max_compute_workgroup_size_x
                         : dev->limits.max_compute_invocations_per_workgroup;
    uint32_t wg = desc->workgroup_size ? desc->workgroup_size : limit;
    if (wg > limit)
        return gs_fail(GS_ERR_WORKGROUP_SIZE_EXCEEDS_LIMIT, wg, limit, 0,
                    "workgroup size exceeds device limit: %u > %u", wg, limit);
    uint32_t total = 0;
    for (uint32_t i = 0; i < desc->bind_group_count; i++) total += desc->bindings_per_group[i];
    if (total > (uint32_t)gs::MAX_BINDINGS)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, total, gs::MAX_BINDINGS, 0, "too many bindings");
    gs_bundle *b = new gs_bundle();
    b->dev = dev;
    b->label = desc->label ? desc->label : "";
    b->kernel = desc->kernel;
    b->sh = desc->sh;
    b->cov = desc->cov;
    b->workgroup_size = wg;
    b->layout.assign(desc->bindings_per_group, desc->bindings_per_group + desc->bind_group_count);
    for (uint32_t i = 0; i < desc->constant_count; i++) {
        if (desc->constant_names && desc->constant_names[i] &&
            !std::strcmp(desc->constant_names[i], "additional_constant")) {
            b->has_additional_constant = true;
            b->additional_constant = (uint32_t)desc->constant_values[i];
        }
    }
    *out = b;
    return GS_OK;
}

extern "C" gs_status gs_bundle_set_bind_group(gs_bundle *b, uint32_t index, gs_buffer *const *buffers,
                                              uint32_t count) {
    if (!b) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null bundle");
    if (index >= b->groups.size())
        return gs_fail(GS_ERR_INVALID_ARGUMENT, index, b->groups.size(), 0, "bind group index out of bounds");
    if (count != b->layout[index])
        return gs_fail(GS_ERR_INVALID_ARGUMENT, count, b->layout[index], 0,
                    "bind group %u expects %u bindings, got %u", index, b->layout[index], count);
    std::vector<gs_buffer *> g;
    for (uint32_t i = 0; i < count; i++) {
        if (!buffers[i]) {
            release_group(g);
            return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null binding");
        }
        g.push_back(gs_buffer_retain(buffers[i]));
    }
    release_group(b->groups[index]);
    b->groups[index] = g;
    return GS_OK;
}

extern "C" gs_status gs_bundle_create_with_bind_groups(gs_device *dev, const gs_bundle_desc *desc,
                                                       gs_buffer *const *const *resources,
                                                       const uint32_t *resource_counts,
                                                       uint32_t resource_group_count,
                                                       gs_bundle **out) {
    gs_bundle *created = nullptr;
    GS_TRY(gs_bundle_create(dev, desc, &created));
    std::unique_ptr<gs_bundle> b(created);
    // compute_bundle.rs:161-168
    if (resource_group_count != b->layout.size())
        return gs_fail(GS_ERR_RESOURCE_COUNT_MISMATCH, resource_group_count, b->layout.size(), 0,
                    "resource count and bind group layout count mismatch: %u != %zu",
                    resource_group_count, b->layout.size());
    b->managed = true;
    b->groups.resize(b->layout.size());
    for (uint32_t i = 0; i < resource_group_count; i++)
        GS_TRY(gs_bundle_set_bind_group(b.get(), i, resources[i], resource_counts[i]));
    *out = b.release();
    return GS_OK;
}

extern "C" void gs_bundle_destroy(gs_bundle *b) {
    delete b;      // (takes the device only when there is a module to unload, as it always did)
}

extern "C" gs_status gs_bundle_create_from_source(gs_device *dev, const gs_bundle_source_desc *desc,
                                                  gs_bundle **out) {
    if (!dev || !desc || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    // same order of checks as ComputeBundleBuilder::build (compute_bundle.rs:505-519)
    if (desc->bind_group_count == 0 || !desc->bindings_per_group)
        return gs_fail(GS_ERR_MISSING_BIND_GROUP_LAYOUT, 0, 0, 0, "missing bind group layout for compute bundle");
    if (!desc->entry_point) return gs_fail(GS_ERR_MISSING_ENTRY_POINT, 0, 0, 0, "missing entry point for compute bundle");
    if (!desc->source) return gs_fail(GS_ERR_MISSING_MAIN_SHADER, 0, 0, 0, "missing main shader for compute bundle");
    if (!valid_cfg(desc->sh, desc->cov)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bad config");
    uint32_t limit = dev->limits.max_compute_workgroup_size_x <
                             dev->limits.max_compute_invocations_per_workgroup
                         ? dev->limits.max_compute_workgroup_size_x
                         : dev->limits.max_compute_invocations_per_workgroup;
    uint32_t wg = desc->workgroup_size ? desc->workgroup_size : limit;
    if (wg > limit)
        return gs_fail(GS_ERR_WORKGROUP_SIZE_EXCEEDS_LIMIT, wg, limit, 0,
                    "workgroup size exceeds device limit: %u > %u", wg, limit);
    uint32_t total = 0;
    for (uint32_t i = 0; i < desc->bind_group_count; i++) total += desc->bindings_per_group[i];
    if (total > (uint32_t)gs::MAX_BINDINGS)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, total, gs::MAX_BINDINGS, 0, "too many bindings");
    GS_TRY(use_device(dev));

    std::vector<std::string> opts;
    opts.push_back(std::string("--offload-arch=") + dev->limits.arch_name);
    opts.push_back("-std=c++17");
    opts.push_back("-ffp-contract=off");
    opts.push_back("-DGS_SH=" + std::to_string((int)desc->sh));
    opts.push_back("-DGS_COV=" + std::to_string((int)desc->cov));
    opts.push_back(std::string("-D") + gs_feature_name((uint32_t)desc->sh) + "=1");
    opts.push_back(std::string("-D") + gs_feature_name(4u + (uint32_t)desc->cov) + "=1");
    opts.push_back("-Dworkgroup_size=" + std::to_string(wg));
    for (uint32_t i = 0; i < desc->define_count; i++)
        if (desc->defines && desc->defines[i]) opts.push_back(std::string("-D") + desc->defines[i] + "=1");
    for (uint32_t i = 0; i < desc->constant_count; i++) {
        if (!desc->constant_names || !desc->constant_names[i]) continue;
        double v = desc->constant_values[i];
        char buf[64];
        if (v == (double)(long long)v) std::snprintf(buf, sizeof(buf), "%lld", (long long)v);
        else std::snprintf(buf, sizeof(buf), "%.17g", v);
        opts.push_back(std::string("-D") + desc->constant_names[i] + "=" + buf);
    }
    std::string entry = desc->entry_point;
    opts.push_back("-Dmain=gs_entry_main");   // `main` cannot name a kernel in C++: always renamed
    if (entry == "main") entry = "gs_entry_main";
    std::vector<const char *> copts;
    for (auto &o : opts) copts.push_back(o.c_str());

    hiprtcProgram prog;
    const char *hdr_src[1] = {k_kernel_lib_src};
    const char *hdr_names[1] = {"wgpu_3dgs_core.h"};
    hiprtcResult rr = hiprtcCreateProgram(&prog, desc->source, "main_shader.hip", 1, hdr_src, hdr_names);
    if (rr != HIPRTC_SUCCESS)
        return gs_fail(GS_ERR_KERNEL_COMPILE, (uint64_t)rr, 0, 0, "hiprtcCreateProgram: %s", hiprtcGetErrorString(rr));
    rr = hiprtcCompileProgram(prog, (int)copts.size(), copts.data());
    if (rr != HIPRTC_SUCCESS) {
        size_t n = 0;
        (void)hiprtcGetProgramLogSize(prog, &n);
        std::string log(n ? n : 1, '\0');
        if (n) (void)hiprtcGetProgramLog(prog, &log[0]);
        (void)hiprtcDestroyProgram(&prog);
        // keep the first error lines
        size_t e = log.find("error");
        std::string shown = e == std::string::npos ? log : log.substr(e > 80 ? e - 80 : 0);
        return gs_fail(GS_ERR_KERNEL_COMPILE, (uint64_t)rr, 0, 0, "kernel compilation failed: %.200s", shown.c_str());
    }
    size_t code_size = 0;
    (void)hiprtcGetCodeSize(prog, &code_size);
    std::vector<char> code(code_size);
    (void)hiprtcGetCode(prog, code.data());
    (void)hiprtcDestroyProgram(&prog);

    std::unique_ptr<gs_bundle> b(new gs_bundle());
    b->dev = dev;
    b->label = desc->label ? desc->label : "";
    b->sh = desc->sh;
    b->cov = desc->cov;
    b->workgroup_size = wg;
    b->layout.assign(desc->bindings_per_group, desc->bindings_per_group + desc->bind_group_count);
    b->from_source = true;
    hipError_t he = hipModuleLoadData(&b->module, code.data());
    if (he == hipSuccess) he = hipModuleGetFunction(&b->func, b->module, entry.c_str());
    if (he != hipSuccess)
        return gs_fail(GS_ERR_MISSING_ENTRY_POINT, (uint64_t)he, 0, 0, "entry point '%s' not found in the compiled module: %s",
                    desc->entry_point, hipGetErrorString(he));
    *out = b.release();
    return GS_OK;
}

// bind groups for a bundle created without them (gs_bundle_create / _from_source): makes it managed
extern "C" gs_status gs_bundle_attach_bind_groups(gs_bundle *b, gs_buffer *const *const *resources,
                                                  const uint32_t *resource_counts,
                                                  uint32_t resource_group_count) {
    if (!b) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null bundle");
    if (resource_group_count != b->layout.size())
        return gs_fail(GS_ERR_RESOURCE_COUNT_MISMATCH, resource_group_count, b->layout.size(), 0,
                    "resource count and bind group layout count mismatch: %u != %zu",
                    resource_group_count, b->layout.size());
    b->managed = true;
    b->groups.resize(b->layout.size());
    for (uint32_t i = 0; i < resource_group_count; i++)
        GS_TRY(gs_bundle_set_bind_group(b, i, resources[i], resource_counts[i]));
    return GS_OK;
}

extern "C" uint32_t gs_bundle_workgroup_size(const gs_bundle *b) { return b ? b->workgroup_size : 0; }
extern "C" const char *gs_bundle_label(const gs_bundle *b) {
    return (b && !b->label.empty()) ? b->label.c_str() : nullptr;
}
extern "C" uint32_t gs_bundle_bind_group_layout_count(const gs_bundle *b) {
    return b ? (uint32_t)b->layout.size() : 0;
}
extern "C" uint32_t gs_bundle_bind_group_count(const gs_bundle *b) {
    return b ? (uint32_t)b->groups.size() : 0;
}
extern "C" uint32_t gs_bundle_last_workgroup_count(const gs_bundle *b) {
    return b ? b->last_workgroups : 0;
}

// minimum byte size each binding must have so that the kernel cannot run out of bounds
static gs_status validate_bindings(const gs_bundle *b, const gs::BundleArgs &a, uint32_t nbind) {
    auto need = [&](uint32_t i, uint64_t bytes) -> gs_status {
        if (i >= nbind || a.size[i] < bytes)
            return gs_fail(GS_ERR_INVALID_ARGUMENT, i, i < nbind ? a.size[i] : 0, bytes,
                        "binding %u is smaller than the %llu bytes the kernel accesses", i,
                        (unsigned long long)bytes);
        return GS_OK;
    };
    uint64_t pod = (uint64_t)gs::pod_bytes(b->sh, b->cov);
    switch (b->kernel) {
    case GS_KERNEL_ARRAY_MAP_ADD:
        GS_TRY(need(0, 0));
        if (b->layout.size() > 1) GS_TRY(need(1, 4));
        break;
    case GS_KERNEL_TEST_GAUSSIAN:
        GS_TRY(need(0, pod));
        GS_TRY(need(1, 56 * 4));
        break;
    case GS_KERNEL_TEST_GAUSSIAN_TRANSFORM:
        GS_TRY(need(0, 8));
        GS_TRY(need(1, 16));
        break;
    case GS_KERNEL_TEST_MODEL_TRANSFORM:
        GS_TRY(need(0, 48));
        GS_TRY(need(1, 12));
        GS_TRY(need(2, 44 * 4));
        break;
    case GS_KERNEL_UNPACK_SOA:
        GS_TRY(need(0, 0));
        GS_TRY(need(1, (a.size[0] / pod) * 55 * 4));
        break;
    default: break;
    }
    return GS_OK;
}

static gs_status dispatch_groups(gs_bundle *b, gs_stream *s, uint32_t count,
                                 const std::vector<std::vector<gs_buffer *>> &groups) {
    if (!s) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null stream");
    if (groups.size() != b->layout.size())
        return gs_fail(GS_ERR_INVALID_ARGUMENT, groups.size(), b->layout.size(), 0,
                    "dispatch needs %zu bind groups, got %zu", b->layout.size(), groups.size());
    gs::BundleArgs a;
    std::memset(&a, 0, sizeof(a));
    uint32_t n = 0;
    for (size_t gi = 0; gi < groups.size(); gi++) {
        if (groups[gi].size() != b->layout[gi])
            return gs_fail(GS_ERR_INVALID_ARGUMENT, groups[gi].size(), b->layout[gi], 0,
                        "bind group %zu is not set or has the wrong binding count", gi);
        for (gs_buffer *buf : groups[gi]) {
            a.ptr[n] = buf->ptr;
            a.size[n] = buf->bytes;
            n++;
        }
    }
    a.reg_second_group = b->layout.size() > 1 ? 1u : 0u;
    a.reg_has_constant = b->has_additional_constant ? 1u : 0u;
    a.reg_constant = b->additional_constant;
    if (!b->from_source) GS_TRY(validate_bindings(b, a, n));
    GS_TRY(use_device(b->dev));
    // compute_bundle.rs:131 — dispatch_workgroups(count.div_ceil(workgroup_size), 1, 1)
    uint32_t wgs = count / b->workgroup_size + (count % b->workgroup_size != 0);
    b->last_workgroups = wgs;
    if (wgs == 0) return GS_OK;
    if (b->from_source) {
        struct { gs::BundleArgs a; uint32_t count; } params{a, count};
        size_t psize = sizeof(params);
        void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &params, HIP_LAUNCH_PARAM_BUFFER_SIZE, &psize,
                          HIP_LAUNCH_PARAM_END};
        GS_HIP(hipModuleLaunchKernel(b->func, wgs, 1, 1, b->workgroup_size, 1, 1, 0, s->s, nullptr, config));
        return GS_OK;
    }
    bundle_kernel_fn fn = nullptr;
    switch (b->kernel) {
    case GS_KERNEL_ARRAY_MAP_ADD: fn = gs::k_array_map_add; break;
    case GS_KERNEL_TEST_GAUSSIAN: fn = k_tbl_test_gaussian[b->sh][b->cov]; break;
    case GS_KERNEL_TEST_GAUSSIAN_TRANSFORM: fn = gs::k_test_gaussian_transform; break;
    case GS_KERNEL_TEST_MODEL_TRANSFORM: fn = gs::k_test_model_transform; break;
    case GS_KERNEL_UNPACK_SOA: fn = k_tbl_unpack_soa[b->sh][b->cov]; break;
    default: return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bad kernel");
    }
    hipLaunchKernelGGL(fn, dim3(wgs), dim3(b->workgroup_size), 0, s->s, a, count);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

extern "C" gs_status gs_bundle_dispatch(gs_bundle *b, gs_stream *s, uint32_t count) {
    if (!b) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null bundle");
    if (!b->managed)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0,
                    "bundle was created without bind groups: use gs_bundle_dispatch_with_bind_groups");
    return dispatch_groups(b, s, count, b->groups);
}

extern "C" gs_status gs_bundle_dispatch_with_bind_groups(gs_bundle *b, gs_stream *s, uint32_t count,
                                                         gs_buffer *const *const *groups,
                                                         const uint32_t *group_counts,
                                                         uint32_t group_count) {
    if (!b || (group_count && (!groups || !group_counts)))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    std::vector<std::vector<gs_buffer *>> gv(group_count);
    for (uint32_t i = 0; i < group_count; i++) {
        for (uint32_t k = 0; k < group_counts[i]; k++) {
            if (!groups[i][k]) return gs_fail(GS_ERR_INVALID_ARGUMENT, i, k, 0, "null binding");
            gv[i].push_back(groups[i][k]);
        }
    }
    return dispatch_groups(b, s, count, gv);
}
