// gs_simplify_kernels.h — merge the Gaussians of each grid cell into one (include/gs3d.h gs_gaussians_buffer_create_simplified;
// DESIGN.md §3.17).  No reference item: the reference has no decimation.
//
// Behind the front of gs_neighbors.hip the Gaussians are sorted by cell key, stable in caller index, so a CELL is a run of
// equal keys.  Three kernels:
//   k_sm_count   the heads of the runs per 256 slots; the library's exclusive scan makes a cell index per slot and K of it
//   k_sm_merge   one lane per sorted slot: gather the record, decode, form the weighted terms, reduce them over the wave
//                SEGMENTED by run (a Hillis-Steele ladder of six shuffle steps: a fixed shape), finalise and encode every
//                run that lies inside the wave; a run that crosses a wave boundary leaves its per-wave partial in the scratch
//   k_sm_long    one wave per such run: its partials are summed 64 at a time (a butterfly per chunk, the chunks in
//                ascending wave order), then finalised and encoded by the same function
// The weights of a cell are alpha_i s_i unless their sum is not > 0 or one of them is not finite; whether that is so is known
// only once the cell is summed.  So k_sm_merge and k_sm_long run TWICE: the first pass sums with alpha_i s_i and marks the
// cells that fail (redo[cell]), the second sums those cells again with unit weights; a wave of the second pass that holds
// no marked cell returns after reading one word per lane.
//
// The sums are binary32 in a shape that depends only on the sorted order: the same input gives the same bytes on every
// call.  The shape is not part of the definition: merged cells are tested against a binary64 witness
// within (m + 16) 2^-24 sum w |t| / W, singleton cells (convert_words / decompose_words, the host's code) bit for bit.
// Every operation is rounded (-ffp-contract=off).
#pragma once

#include "gs_neighbor_grid.h"
#include "gs_pack_kernels.h"

namespace gs {

// the terms of a cell: W, 3 first moments, 6 second moments (about the cell centre), 3 colours, 45 SH coefficients and the
// sum of w alpha (the opacity of the unit-weight fallback)
constexpr int SM_W = 0, SM_D = 1, SM_S = 4, SM_RGB = 10, SM_SH = 13, SM_ALPHA = 58, SM_TERMS = 59;
// a partial of the scratch: the terms, then the cell and what the partial is; two per wave of slots: [0] the run that
// came in from the wave before, [1] the run that starts here and goes on into the next wave
constexpr uint32_t SM_PART_WORDS = 64u, SM_PART_CELL = 60u, SM_PART_STATE = 61u;
enum : uint32_t { SM_NONE = 0u, SM_OPEN = 1u, SM_MIDDLE = 2u, SM_LAST = 3u };

__device__ __forceinline__ bool sm_head(const uint64_t *__restrict__ keys, uint32_t s, uint32_t n) {
    if (s >= n) return false;
    const uint64_t k = keys[s];
    return k != NB_KEY_NONE && (s == 0u || keys[s - 1u] != k);
}

// counts[block] = the runs that start in the block's 256 slots
__global__ __launch_bounds__(256) void k_sm_count(const uint64_t *__restrict__ keys, uint32_t n, uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_c[4];
    const uint32_t s = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t hb = __ballot(sm_head(keys, s, n));
    if (lane == 0u) s_c[wid] = (uint32_t)__popcll(hb);
    __syncthreads();
    if (threadIdx.x == 0u) counts[blockIdx.x] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
}

// the centre of the cell `key` per axis: lo + (cell + 0.5) h in binary64, rounded to binary32
__device__ __forceinline__ void sm_cell_centre(const float *__restrict__ bbox, float cell_size, uint64_t key, float c[3]) {
    double lo[3];
    const double h = nb_grid_side(bbox, cell_size, lo);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const uint32_t q = (uint32_t)(key >> (NB_CELL_BITS * (uint32_t)a)) & NB_CELL_MAX;
        c[a] = (float)(lo[a] + ((double)q + 0.5) * h);
    }
}

// The summed terms of a cell of m >= 2 members -> its record of layout (DSH, dcov) at `rec`.  Returns false,
// and writes nothing, where the weights alpha s do not serve (W not > 0; a weight that is not finite has made W a NaN): the
// cell is summed again with UNIT weights, which always serve.
template <int DSH>
__device__ __forceinline__ bool sm_finalise(const float t[SM_TERMS], bool unit, const float c[3], int dcov, uint4 *__restrict__ rec) {
    const float W = t[SM_W];
    if (!unit && !(W > 0.0f)) return false;
    uint32_t r[56], o[56];
    const float dx = t[SM_D] / W, dy = t[SM_D + 1] / W, dz = t[SM_D + 2] / W;
    r[0] = f2u(c[0] + dx);
    r[1] = f2u(c[1] + dy);
    r[2] = f2u(c[2] + dz);
    float S[6] = {t[SM_S] / W - dx * dx,     t[SM_S + 1] / W - dx * dy, t[SM_S + 2] / W - dx * dz,
                  t[SM_S + 3] / W - dy * dy, t[SM_S + 4] / W - dy * dz, t[SM_S + 5] / W - dz * dz};
    S[0] = S[0] < 0.0f ? 0.0f : S[0];
    S[3] = S[3] < 0.0f ? 0.0f : S[3];
    S[5] = S[5] < 0.0f ? 0.0f : S[5];
    const float trace = (S[0] + S[3]) + S[5];
    const float alpha = unit ? t[SM_ALPHA] / W : (trace > 0.0f ? W / trace : 0.0f);
    uint32_t color = cv_sat_u8(255.0f * cv_clamp(alpha, 0.0f, 1.0f) + 0.5f) << 24;
#pragma unroll
    for (int k = 0; k < 3; k++) color |= cv_sat_u8(255.0f * (t[SM_RGB + k] / W) + 0.5f) << (8 * k);
    r[3] = color;
#pragma unroll
    for (int k = 0; k < 45; k++) r[4 + k] = f2u(t[SM_SH + k] / W);
#pragma unroll
    for (int k = 0; k < 6; k++) r[49 + k] = f2u(S[k]);
    r[55] = 0u;
    constexpr int DNC_MAX = pod_words(DSH, COV_ROT_SCALE) / 4;
    const int dnc = pod_words(DSH, dcov) / 4;
    if (DSH == SH_SINGLE && dcov == COV_SINGLE) {
#pragma unroll
        for (int k = 0; k < 56; k++) o[k] = r[k];
    } else if (dcov == COV_ROT_SCALE) {
        decompose_words(SH_SINGLE, COV_SINGLE, DSH, r, o, DeviceSqrt());
    } else {
        convert_words(SH_SINGLE, COV_SINGLE, DSH, dcov, r, o);
    }
#pragma unroll
    for (int q = 0; q < DNC_MAX; q++)
        if (q < dnc) rec[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    return true;
}

// One lane per sorted slot, 64 consecutive slots per wave (see the head of the file).  offsets[block]: the cells that start
// before the block (k_sm_count, scanned).  UNIT pass: only the cells with redo[cell] != 0 are summed and written.
// cell_of (first pass, may be null): cell_of[vals[s]] = the cell of slot s, 0xffffffff where the slot holds no point.
// part: 2 partials per wave of slots.  A cell index is < K <= the records of dst by construction (K is the scan's total).
template <int SSH, int DSH>
__global__ __launch_bounds__(256) void k_sm_merge(const uint4 *__restrict__ src, int scov, int dcov, const uint64_t *__restrict__ keys,
                                                  const uint32_t *__restrict__ vals, uint32_t n, const float *__restrict__ bbox,
                                                  float cell_size, const uint32_t *__restrict__ offsets, uint32_t unit,
                                                  uint32_t *__restrict__ redo, uint32_t *__restrict__ part, uint4 *__restrict__ dst,
                                                  uint32_t *__restrict__ cell_of, uint32_t K) {
    constexpr int SNC_MAX = pod_words(SSH, COV_ROT_SCALE) / 4;
    __shared__ uint32_t s_c[4];
    const uint32_t s = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t key = s < n ? keys[s] : NB_KEY_NONE;
    const bool valid = key != NB_KEY_NONE;
    const bool head = valid && (s == 0u || keys[s - 1u] != key);
    const bool last = valid && (s + 1u >= n || keys[s + 1u] != key);
    const uint64_t hb = __ballot(head);
    if (lane == 0u) s_c[wid] = (uint32_t)__popcll(hb);
    __syncthreads();
    uint32_t before = offsets[blockIdx.x];
    for (uint32_t w = 0; w < wid; w++) before += s_c[w];
    // (a valid slot has a head at or before it; the subtraction cannot wrap for one)
    const uint32_t cell = before + mbcnt(hb) + (head ? 1u : 0u) - 1u;
    const uint32_t idx = s < n ? vals[s] : 0u;
    if (!unit && cell_of && s < n) cell_of[idx] = valid ? cell : 0xffffffffu;
    // a run starts at its head, at lane 0 and at every slot without a point; the lane behind which a run leaves the wave
    // will hold the run's terms: the WHOLE run, or a PIECE of one that crosses a wave boundary
    const uint64_t starts = __ballot(head || lane == 0u || !valid);
    const uint32_t first = 63u - (uint32_t)__builtin_clzll(starts & (~0ull >> (63u - lane)));
    const uint32_t dist = lane - first;
    const bool from_here = (hb >> first) & 1ull;
    const bool end = valid && (last || lane == 63u);
    const bool whole = end && from_here && last, piece = end && !whole;
    const uint32_t gw = s >> 6;
    if (!unit && s - lane < n) {      // the partials this wave does not write say so: k_sm_long looks at every wave's (the
                                      // last block may hold waves behind n: they have no partials)
        const bool lead = __any(piece && !from_here), trail = __any(piece && from_here);
        if (lane == 0u && !lead) part[(2u * gw) * SM_PART_WORDS + SM_PART_STATE] = SM_NONE;
        if (lane == 1u && !trail) part[(2u * gw + 1u) * SM_PART_WORDS + SM_PART_STATE] = SM_NONE;
    }
    const bool wanted = valid && cell < K && (!unit || redo[cell] != 0u);
    if (!__any(wanted)) return;

    // the lane's record -> its terms
    const uint32_t snc = (uint32_t)pod_words(SSH, scov) / 4u;
    float t[SM_TERMS];
#pragma unroll
    for (int k = 0; k < SM_TERMS; k++) t[k] = 0.0f;
    uint32_t members = 0u;
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (wanted) {
        const uint4 *rec = src + (uint64_t)idx * snc;
        uint32_t w[SNC_MAX * 4];
#pragma unroll
        for (int q = 0; q < SNC_MAX; q++) {
            const uint4 v = (uint32_t)q < snc ? rec[q] : make_uint4(0u, 0u, 0u, 0u);
            w[4 * q] = v.x;
            w[4 * q + 1] = v.y;
            w[4 * q + 2] = v.z;
            w[4 * q + 3] = v.w;
        }
        sm_cell_centre(bbox, cell_size, key, c);
        float c6[6];
        if (scov == COV_ROT_SCALE) {      // as convert_words makes a covariance of rotation + scale: the host's bits
            const uint32_t *cw = w + cov_word0(SSH);
            const float q[4] = {u2f(cw[0]), u2f(cw[1]), u2f(cw[2]), u2f(cw[3])}, sc[3] = {u2f(cw[4]), u2f(cw[5]), u2f(cw[6])};
            cov3d_from_rot_scale(q, sc, c6);
        } else if (scov == COV_SINGLE) gaussian_unpack_cov3d<SSH, COV_SINGLE>(w, c6);
        else gaussian_unpack_cov3d<SSH, COV_HALF>(w, c6);
        const float alpha = unorm8(w[3], 3);
        float wt = alpha * ((c6[0] + c6[3]) + c6[5]);
        if (!attr_finite(wt)) wt = __builtin_nanf("");      // W becomes a NaN: the cell is summed again with unit weights
        if (unit) wt = 1.0f;
        const float d[3] = {u2f(w[0]) - c[0], u2f(w[1]) - c[1], u2f(w[2]) - c[2]};
        t[SM_W] = wt;
#pragma unroll
        for (int a = 0; a < 3; a++) t[SM_D + a] = wt * d[a];
        t[SM_S] = wt * (c6[0] + d[0] * d[0]);
        t[SM_S + 1] = wt * (c6[1] + d[0] * d[1]);
        t[SM_S + 2] = wt * (c6[2] + d[0] * d[2]);
        t[SM_S + 3] = wt * (c6[3] + d[1] * d[1]);
        t[SM_S + 4] = wt * (c6[4] + d[1] * d[2]);
        t[SM_S + 5] = wt * (c6[5] + d[2] * d[2]);
#pragma unroll
        for (int k = 0; k < 3; k++) t[SM_RGB + k] = wt * unorm8(w[3], k);
#pragma unroll
        for (int k = 0; k < 45; k++) t[SM_SH + k] = wt * u2f(sh_coef_bits(SSH, w + 4, k));
        t[SM_ALPHA] = wt * alpha;
        members = 1u;
    }

    // segmented inclusive scan over the runs
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const bool take = dist >= d;
#pragma unroll
        for (int k = 0; k < SM_TERMS; k++) {
            const float x = __shfl_up(t[k], d, WAVE);
            t[k] = take ? t[k] + x : t[k];
        }
        const uint32_t m = (uint32_t)__shfl_up((int)members, d, WAVE);
        members += take ? m : 0u;
    }

    if (!wanted) return;
    if (piece) {
        uint32_t *p = part + (2u * gw + (from_here ? 1u : 0u)) * SM_PART_WORDS;
#pragma unroll
        for (int k = 0; k < SM_TERMS; k++) p[k] = f2u(t[k]);
        p[SM_PART_CELL] = cell;
        p[SM_PART_STATE] = from_here ? SM_OPEN : last ? SM_LAST : SM_MIDDLE;
    }
    if (!whole) return;
    const uint32_t dnc = (uint32_t)pod_words(DSH, dcov) / 4u;
    uint4 *out = dst + (uint64_t)cell * dnc;
    if (members == 1u) {      // (first pass only: its cell is never marked) the record itself, converted as the host converts it
        constexpr int DNC_MAX = pod_words(DSH, COV_ROT_SCALE) / 4;
        const uint4 *rec = src + (uint64_t)idx * snc;
        uint32_t w[SNC_MAX * 4], o[DNC_MAX * 4];
#pragma unroll
        for (int q = 0; q < SNC_MAX; q++) {
            const uint4 v = (uint32_t)q < snc ? rec[q] : make_uint4(0u, 0u, 0u, 0u);
            w[4 * q] = v.x;
            w[4 * q + 1] = v.y;
            w[4 * q + 2] = v.z;
            w[4 * q + 3] = v.w;
        }
        if (SSH == DSH && scov == dcov) {      // identical layouts keep every byte, the trailing pad too
            if constexpr (SSH == DSH) {
#pragma unroll
                for (int k = 0; k < DNC_MAX * 4; k++) o[k] = w[k];
            }
        } else if (dcov == COV_ROT_SCALE && scov != COV_ROT_SCALE) {
            decompose_words(SSH, scov, DSH, w, o, DeviceSqrt());
        } else {
            convert_words(SSH, scov, DSH, dcov, w, o);
        }
#pragma unroll
        for (int q = 0; q < DNC_MAX; q++)
            if ((uint32_t)q < dnc) out[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
        redo[cell] = 0u;
        return;
    }
    const bool done = sm_finalise<DSH>(t, unit != 0u, c, dcov, out);
    if (!unit) redo[cell] = done ? 0u : 1u;
}

// One wave per wave of slots `g`: where a run starts there and goes on (partial [1] of g is SM_OPEN), the wave sums that
// partial and partials [0] of the waves g + 1, g + 2, ... up to the run's SM_LAST, 64 partials at a time — lane j takes
// partial j of the chunk, a butterfly sums the chunk, the chunks are added in ascending order — and lane 0 finalises.
// The run of g ends in lane 63 of g, which is where its key is read.  nwaves bounds the walk whatever the states say.
template <int DSH>
__global__ __launch_bounds__(256) void k_sm_long(const uint32_t *__restrict__ part, uint32_t n, int dcov,
                                                 const uint64_t *__restrict__ keys, const float *__restrict__ bbox, float cell_size,
                                                 uint32_t unit, uint32_t *__restrict__ redo, uint4 *__restrict__ dst, uint32_t K) {
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = (n + 63u) / 64u;
    if (g >= nwaves) return;
    const uint32_t *p0 = part + (2u * g + 1u) * SM_PART_WORDS;
    if (p0[SM_PART_STATE] != SM_OPEN) return;
    const uint32_t cell = p0[SM_PART_CELL];
    if (cell >= K || (unit && redo[cell] == 0u)) return;
    float total[SM_TERMS];
#pragma unroll
    for (int k = 0; k < SM_TERMS; k++) total[k] = 0.0f;
    bool more = true;
    for (uint32_t j0 = 0u; more; j0 += 64u) {
        const uint32_t j = j0 + lane;      // element 0: the open partial of g; element j: partial [0] of wave g + j
        const bool inside = j < nwaves - g;
        const uint32_t *p = j == 0u ? p0 : part + (2u * (g + (inside ? j : 0u))) * SM_PART_WORDS;
        const uint32_t state = inside ? p[SM_PART_STATE] : SM_NONE;
        const uint64_t stop = __ballot(j != 0u && state != SM_MIDDLE);
        const uint32_t upto = stop ? (uint32_t)__builtin_ctzll(stop) : 63u;
        const bool take = lane <= upto && (j == 0u || state == SM_MIDDLE || state == SM_LAST);
        more = stop == 0ull;
#pragma unroll
        for (int k = 0; k < SM_TERMS; k++) {
            float v = take ? u2f(p[k]) : 0.0f;
#pragma unroll
            for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
            total[k] += v;
        }
    }
    if (lane != 0u) return;
    float c[3];
    sm_cell_centre(bbox, cell_size, keys[g * 64u + 63u < n ? g * 64u + 63u : n - 1u], c);
    const uint32_t dnc = (uint32_t)pod_words(DSH, dcov) / 4u;
    const bool done = sm_finalise<DSH>(total, unit != 0u, c, dcov, dst + (uint64_t)cell * dnc);
    if (!unit) redo[cell] = done ? 0u : 1u;
}

}  // namespace gs
