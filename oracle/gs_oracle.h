/*
 * gs_oracle.h — CPU ORACLE for the 3DGS render hot path.  TEST INFRASTRUCTURE ONLY.
 *
 * This library is the *checker*: only tests/, __graft_entry__.smoke() and bench.py's
 * `cpu_baseline` leg may load it.  Nothing under wgpu-3dgs-core_amd/ links, imports or
 * calls it, and the product path has no CPU fallback.
 *
 * What it restates (citations relative to /root/reference, LioQing/wgpu-3dgs-core v0.6.0):
 *   - Gaussian record ......................... src/gaussian.rs:53-60
 *   - 12 GaussianPod layouts .................. src/buffer/gaussian.rs:301-384
 *   - SH / cov3d encoders ..................... src/gaussian_config.rs:32-233
 *   - WESL unpack functions ................... src/shader/gaussian.wesl:24-149
 *   - transform flags ......................... src/shader/gaussian_transform.wesl:4-31,
 *                                               src/buffer/gaussian_transform.rs:55-98,166-206
 *   - model matrices .......................... src/shader/model_transform.wesl:6-143,
 *                                               src/buffer/model_transform.rs:61-84
 *   - test fixture given::gaussian_with_seed .. tests/common/given.rs:48-81
 *   - SPZ columns + from_spz / to_spz ......... src/source_format/spz.rs:436-794, src/gaussian.rs:126-352
 *   - Inria PLY record + from_ply ............. src/source_format/ply.rs:11-21,204-267,
 *                                               src/gaussian.rs:70-92
 *
 * PARITY STATUS
 *   Rows a1-a14 (everything above): pinned — checked against the known-answer values of the
 *   reference's own tests (tests/shader/ and src/buffer/gaussian.rs:386-527) and against golden
 *   vectors produced by an independent numpy restatement (tests/golden/make_golden.py).
 *   Rows x1-x5 (SH evaluation, projection, key build, sort, blend): *** PARITY UNPINNED ***.
 *   These stages do not exist in the reference (they live in the downstream wgpu-3dgs-viewer,
 *   which is not on this machine); this file is their normative definition (Kerbl et al. 2023
 *   formulas in this crate's conventions).
 *
 * All arithmetic is IEEE binary32, evaluated in the written order, never contracted
 * (-ffp-contract=off) except where fmaf() is written explicitly.
 */
#ifndef GS_ORACLE_H
#define GS_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { GSO_SH_SINGLE = 0, GSO_SH_HALF = 1, GSO_SH_NORM8 = 2, GSO_SH_NONE = 3 };
enum { GSO_COV_ROT_SCALE = 0, GSO_COV_SINGLE = 1, GSO_COV_HALF = 2 };

/* src/gaussian.rs:53-60 — rot is xyzw. 224 bytes, no padding. */
typedef struct {
    float rot[4];
    float pos[3];
    uint8_t color[4];
    float sh[45];
    float scale[3];
} gso_gaussian;

/* src/buffer/gaussian_transform.rs:166-174 */
typedef struct {
    float size;
    uint8_t flags[4]; /* display_mode, sh_deg, no_sh0, max_std_dev_u8 */
} gso_gaussian_transform;

/* src/buffer/model_transform.rs:61-66 (Vec3A = 16 bytes) */
typedef struct {
    float pos[3];
    float _pad0;
    float rot[4];
    float scale[3];
    float _pad1;
} gso_model_transform;

/* src/source_format/ply.rs:11-21 */
typedef struct {
    float pos[3];
    float normal[3];
    float color[3];
    float sh[45];
    float alpha;
    float scale[3];
    float rot[4]; /* wxyz */
} gso_ply_pod;

/* EXTERNAL spec. view is column-major world->view, right-handed, -Z forward. */
typedef struct {
    float view[16];
    float pos[3];
    float fx, fy, cx, cy;
    float near_plane, far_plane;
    uint32_t width, height;
    float background[3];
} gso_camera;

/* Projected splat record: conic is stored pre-scaled (-A/2, -B, -C/2). */
typedef struct {
    float mx, my;
    float ca, cb, cc;
    float opacity;
    float r, g, b;
    float depth;
    uint16_t tx0, ty0, tx1, ty1;
} gso_projected;

/* ---- rows a2-a9: layouts and encoders ---- */
size_t gso_pod_size(int sh, int cov);
size_t gso_sh_bytes(int sh);
size_t gso_cov_bytes(int cov);
void gso_pod_features(int sh, int cov, int out[7]);
void gso_pack(int sh, int cov, const gso_gaussian *in, size_t n, void *out);
/* returns 0, or -1 when the config cannot be inverted (reference panics) */
int gso_unpack_to_gaussian(int sh, int cov, const void *pods, size_t n, gso_gaussian *out);

/* ---- rows a3-a10: WESL functions ---- */
void gso_unpack_color(const void *pod, float out[4]);
void gso_unpack_sh(int sh, const void *pod, uint32_t sh_index, float out[3]);
void gso_unpack_cov3d(int sh, int cov, const void *pod, float out[6]);
/* tests/shader/gaussian.rs:26-59 harness: color[4], sh[45], cov3d[6], pad -> 56 floats */
void gso_shader_test_gaussian(int sh, int cov, const void *pod, float out[56]);

/* ---- row a11 ---- */
int gso_max_std_dev_encode(float v, uint8_t *out);      /* -1 if outside [0,3] */
int gso_gaussian_transform_new(float size, uint32_t mode, uint32_t sh_deg, int no_sh0,
                               float max_std_dev, gso_gaussian_transform *out);
uint32_t gso_transform_display_mode(uint32_t flags);
uint32_t gso_transform_sh_deg(uint32_t flags);
uint32_t gso_transform_no_sh0(uint32_t flags);
float gso_transform_max_std_dev(uint32_t flags);

/* ---- row a12 ---- */
void gso_model_transform_new(const float pos[3], const float rot[4], const float scale[3],
                             gso_model_transform *out);
void gso_model_transform_mat(const gso_model_transform *m, float out[16]); /* column-major */
void gso_model_transform_inv_sr_mat(const gso_model_transform *m, float out[9]);
void gso_model_scale_rot_mat(const gso_model_transform *m, float out[9]);
void gso_model_to_world(const gso_model_transform *m, const float p[3], float out[4]);

/* ---- fixtures ---- */
void gso_given_gaussian_with_seed(uint32_t seed, gso_gaussian *out);
void gso_gaussian_from_ply(const gso_ply_pod *ply, gso_gaussian *out);
void gso_gaussians_from_ply(const gso_ply_pod *ply, size_t n, gso_gaussian *out);
void gso_gaussian_to_ply(const gso_gaussian *g, gso_ply_pod *out);
/* Inria fast-path reader: returns count (>=0) or negative error; out may be NULL to query count */
long gso_read_inria_ply(const uint8_t *bytes, size_t len, gso_ply_pod *out, size_t cap);

/* ---- SPZ (decompressed payload), src/source_format/spz.rs:436-512,739-794 + src/gaussian.rs:126-352.
 * header = 16 bytes {magic u32, version u32, num_points u32, sh_degree u8, fractional_bits u8,
 * flags u8, reserved u8}.  Return: count / byte size (>= 0), -1 bad magic, -2 bad version,
 * -3 bad sh degree, -4 truncated. out may be NULL to query. */
long gso_spz_decode_raw(const uint8_t *bytes, size_t len, gso_gaussian *out, size_t cap);
long gso_spz_encode_raw(const gso_gaussian *in, size_t n, uint32_t version, uint32_t sh_degree,
                        uint32_t fractional_bits, int antialiased, const uint32_t sh_bits[3],
                        uint8_t *out, size_t cap);

/* ---- launch arithmetic, src/compute_bundle.rs:131 ---- */
uint32_t gso_dispatch_workgroups(uint32_t count, uint32_t workgroup_size);

/* ---- rows x1-x5 (EXTERNAL spec) ---- */
float gso_exp(float x);
void gso_camera_look_at(const float eye[3], const float target[3], const float up[3],
                        float vfov_rad, uint32_t width, uint32_t height, float near_plane,
                        float far_plane, gso_camera *out);
/* tiles are 16x16; band = [band_ty0, band_ty1) tile rows owned by this shard */
/* tile_rows (may be NULL; rect version 4): per Gaussian 0 = every tile of the record's rect, or
 * 0x8000 | row code for a rect of at most 3 x 3 tiles some of whose tiles the splat cannot reach — 4 bits per tile
 * row: (first kept column) | (kept columns) << 2; tiles_touched counts the kept tiles */
void gso_preprocess(int sh, int cov, const void *pods, size_t n, const gso_gaussian_transform *gt,
                    const gso_model_transform *mt, const gso_camera *cam, uint32_t band_ty0,
                    uint32_t band_ty1, gso_projected *proj, uint32_t *tiles_touched, uint16_t *tile_rows);
/* keys/idx must hold sum(tiles_touched) entries; returns that sum.  tile_rows as gso_preprocess wrote it (NULL only
 * for frames without dropped tiles: the function aborts when a count and its rect disagree) */
uint64_t gso_build_keys(const gso_projected *proj, const uint32_t *tiles_touched, const uint16_t *tile_rows, size_t n,
                        uint32_t tiles_x, uint64_t *keys, uint32_t *idx);
/* same, emitting in mirror order: order[slot] = Gaussian index (NULL = index order); DESIGN.md §3.4 */
uint64_t gso_build_keys_ordered(const gso_projected *proj, const uint32_t *tiles_touched, const uint16_t *tile_rows,
                                size_t n, uint32_t tiles_x, uint64_t *keys, uint32_t *idx, const uint32_t *order);
/* the spatial mirror order of DESIGN.md §3.4a (30-bit Morton code of the position, ties by index) */
void gso_spatial_order(const void *pods, size_t n, size_t pod_bytes, uint32_t *order);
void gso_sort_pairs(uint64_t *keys, uint32_t *idx, uint64_t d);
/* ranges: 2 u32 per tile [start,end) over tiles_x*tiles_y tiles */
void gso_tile_ranges(const uint64_t *keys, uint64_t d, uint32_t num_tiles, uint32_t *ranges);
/* rgba: height*width*4 floats; only rows of tile rows [band_ty0,band_ty1) are written */
void gso_blend(const gso_projected *proj, const uint32_t *idx, const uint32_t *ranges,
               const gso_camera *cam, uint32_t band_ty0, uint32_t band_ty1, float *rgba);
/* same with GaussianDisplayMode (0 splat, 1 ellipse, 2 point) */
void gso_blend_mode(const gso_projected *proj, const uint32_t *idx, const uint32_t *ranges,
                    const gso_camera *cam, uint32_t band_ty0, uint32_t band_ty1, float *rgba,
                    uint32_t display_mode, float max_std_dev);
/* same, and stopped[height*width]: 1 where the pixel left its list through the transmittance test (test_T < 1e-4), 0 where
 * it ran to the list's end; only pixels of the band are written */
void gso_blend_mode_stopped(const gso_projected *proj, const uint32_t *idx, const uint32_t *ranges,
                            const gso_camera *cam, uint32_t band_ty0, uint32_t band_ty1, float *rgba,
                            uint32_t display_mode, float max_std_dev, uint8_t *stopped);
/* whole frame; optional outputs may be NULL. returns D. */
uint64_t gso_render(int sh, int cov, const void *pods, size_t n, const gso_gaussian_transform *gt,
                    const gso_model_transform *mt, const gso_camera *cam, uint32_t band_ty0,
                    uint32_t band_ty1, float *rgba, uint64_t *visible_out);
uint64_t gso_render_ordered(int sh, int cov, const void *pods, size_t n, const gso_gaussian_transform *gt,
                            const gso_model_transform *mt, const gso_camera *cam, uint32_t band_ty0,
                            uint32_t band_ty1, float *rgba, uint64_t *visible_out,
                            const uint32_t *order);
/* per-stage wall time of the last gso_render on this thread, seconds:
 * preprocess, keys, sort, ranges, blend */
void gso_last_stage_seconds(double out[5]);
void gso_set_threads(int n);
/* tile-rect definition of DESIGN.md §3.3: 1 = radius square, 2 (default) = clipped to the splat's
 * visible box in display mode Splat (same images, fewer pairs) */
void gso_set_rect_version(int v);
int gso_rect_version(void);
int gso_get_max_threads(void);
int gso_effective_threads(void);   /* CPUs this process may run on (affinity mask cut by the cgroup quota) */

#ifdef __cplusplus
}
#endif
#endif
