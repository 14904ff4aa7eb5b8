/* The limit table of the blend's pixel test (k_blend_np_limit in csrc/gs_render_kernels.h).
 *
 * The Splat-mode step decides "alpha >= 1/255" with alpha = min(0.99, fl(op * e)), op = fl(k / 255) for the opacity
 * byte k and e = the blend's own exp of power in [-5.6, -0].  This program restates that exp operation by operation
 * (fmaf, magic-number rounding, the integer-add ldexp), evaluates it at EVERY binary32 of [-5.6, -0] and shows that,
 * although it is not monotone, the set of powers that pass is up-closed for every byte: there is one float L(k) with
 *     pass(k, power)  <=>  -power <= L(k)          for every float power in [-5.6, -0].
 * Below -5.6 nothing passes for any byte (e^-5.6 < 1/255), so the step may test bits(-power) < bits(L(k)) + 1 alone.
 *
 * Two sweeps.  Going down from -0, the running minimum of e gives per byte the first power that fails; going up from
 * -5.6, the running maximum gives the last power that passes.  The pass set is up-closed exactly when the two are
 * adjacent floats, and L(k) is the negated last power that passes.
 *
 * Build and run (host only, no GPU; some 20 s on one core):
 *     mkdir -p build && cc -O2 -ffp-contract=off -o build/blend_alpha_limits tools/blend_alpha_limits.c -lm
 *     build/blend_alpha_limits > profiles/blend_alpha_limits.txt
 * The exit status is non-zero if any byte's pass set is not up-closed.  The 256 words are printed in the layout of the
 * header's table; tests/test_blend_alpha_limit.py checks the header's copy against the oracle's exp.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

#define LIMIT_LO 5.6f   /* the domain of the integer-add ldexp is [-5.6, 0] */

/* GS_BLEND_STEP's exp, from np = -power >= +0: the same roundings in the same order */
static inline float blend_exp(float np) {
    const float tt = np * -1.44269504088896340736f;
    const float tm = tt + 12582912.0f;
    const float n = tm - 12582912.0f;
    const float f = tt - n;
    float p = 0x1.5f0896p-10f;
    p = fmaf(p, f, 0x1.3cbf6cp-7f);
    p = fmaf(p, f, 0x1.c6af6cp-5f);
    p = fmaf(p, f, 0x1.ebfa4ap-3f);
    p = fmaf(p, f, 0x1.62e430p-1f);
    p = fmaf(p, f, 1.0f);
    return u2f(f2u(p) + (f2u(tm) << 23));
}

static int passes(float op, float e) { return fminf(0.99f, op * e) >= 1.0f / 255.0f; }

/* the smallest positive float e that passes for op (fl(op * e) is monotone in e): bisection on the bits */
static float smallest_passing_e(float op) {
    uint32_t lo = 0u, hi = f2u(2.0f);   /* lo fails, hi passes */
    if (!passes(op, u2f(hi))) return INFINITY;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (passes(op, u2f(mid))) hi = mid; else lo = mid;
    }
    return u2f(hi);
}

typedef struct { float emin; int k; } thr_t;
static int by_emin_desc(const void *a, const void *b) {
    const float x = ((const thr_t *)a)->emin, y = ((const thr_t *)b)->emin;
    return x < y ? 1 : x > y ? -1 : 0;
}

int main(void) {
    const uint32_t top = f2u(LIMIT_LO);      /* np runs over the bit patterns 0 .. top: +0 .. 5.6 */
    thr_t thr[255];
    float emin[256];
    for (int k = 1; k < 256; k++) {
        const float op = (float)k / 255.0f;
        if ((uint32_t)(255.0f * op + 0.5f) != (uint32_t)k) {
            fprintf(stderr, "kop does not return byte %d\n", k);
            return 2;
        }
        emin[k] = smallest_passing_e(op);
        thr[k - 1].emin = emin[k];
        thr[k - 1].k = k;
    }
    qsort(thr, 255, sizeof(thr_t), by_emin_desc);

    /* sweep 1, np upwards: first np that fails, per byte; adjacent-float inversions of the exp on the way */
    uint32_t first_fail[256], last_pass[256];
    for (int k = 0; k < 256; k++) first_fail[k] = top + 1u, last_pass[k] = 0xfffffff0u;   /* none */
    uint64_t inversions = 0, out_of_order = 0;
    double worst_drop = 0.0;
    uint32_t worst_at = 0u;
    {
        int at = 0;   /* thr[at..] have not failed yet */
        float run_min = INFINITY, prev = INFINITY;
        for (uint32_t b = 0u; b <= top; b++) {
            const float e = blend_exp(u2f(b));
            if (e > prev) {   /* power fell by one ulp and the exp rose */
                inversions++;
                const double drop = ((double)e - (double)prev) / (double)e;
                if (drop > worst_drop) worst_drop = drop, worst_at = b;
            }
            prev = e;
            if (e < run_min) {
                run_min = e;
                while (at < 255 && run_min < thr[at].emin) first_fail[thr[at++].k] = b;
            }
        }
    }
    /* sweep 2, np downwards: last np that passes, per byte (the running maximum of e rises; bytes in ascending emin) */
    {
        int at = 254;   /* thr[..at] have not passed yet */
        float run_max = -INFINITY;
        for (uint32_t b = top;; b--) {
            const float e = blend_exp(u2f(b));
            if (e < run_max) out_of_order++;   /* a more negative power has the larger exp */
            if (e > run_max) {
                run_max = e;
                while (at >= 0 && run_max >= thr[at].emin) last_pass[thr[at--].k] = b;
            }
            if (b == 0u) break;
        }
    }

    /* up-closed: the last pass lies just below the first failure, and np = +0 passes */
    int bad = 0;
    uint32_t limit[256];
    limit[0] = 0u;
    for (int k = 1; k < 256; k++) {
        if (first_fail[k] == 0u || last_pass[k] + 1u != first_fail[k]) bad++;
        limit[k] = first_fail[k];                                      /* bits(L(k)) + 1 */
    }
    printf("# floats scanned in [-5.6, -0]: %u\n", top + 1u);
    printf("# adjacent-float inversions of the exp (it rises where power falls by one ulp): %llu\n", (unsigned long long)inversions);
    printf("# floats whose exp lies below that of some more negative power: %llu\n", (unsigned long long)out_of_order);
    printf("# worst relative drop: %.3g at power = -%.9g\n", worst_drop, (double)u2f(worst_at));
    printf("# bytes whose pass set is not up-closed: %d\n", bad);
    float lmax = 0.0f;
    for (int k = 1; k < 256; k++) if (u2f(limit[k] - 1u) > lmax) lmax = u2f(limit[k] - 1u);
    printf("# largest L(k): %.9g\n", (double)lmax);
    printf("# k_blend_np_limit[256]: bits(L(k)) + 1, entry 0 = 0\n");
    for (int k = 0; k < 256; k += 8) {
        printf("   ");
        for (int q = 0; q < 8; q++) printf(" 0x%08xu,", limit[k + q]);
        printf("\n");
    }
    printf("# k, L(k), smallest passing e\n");
    for (int k = 1; k < 256; k++) printf("# %3d %.9g %.9g\n", k, (double)u2f(limit[k] - 1u), (double)emin[k]);
    return bad ? 1 : 0;
}
