// gs_align_fit.h — the host arithmetic of gs_rigid_fit and gs_model_transform_compose (include/gs3d.h; no
// reference item): binary64, no device, no HIP, no allocation.  gs_align.hip wraps the two functions into the C ABI;
// tests/cpp/align_fit_sanitized.cpp includes this header alone and runs it under the address and undefined-behaviour
// sanitizers on the CPU.
#pragma once

#include "../../include/gs3d.h"

#include <cmath>

namespace gsfit {

constexpr int JACOBI_SWEEPS = 12;      // fixed, as gs_cov3d_decompose fixes its six: a 4 x 4 matrix is diagonal to the last bit long before
// the rotation is undetermined when the two largest eigenvalues of N are closer than this part of its Frobenius norm
constexpr double GAP_MIN = 0x1p-40;

// Cyclic Jacobi on the symmetric 4 x 4 matrix a (destroyed): JACOBI_SWEEPS sweeps over the six pairs (0,1) (0,2) (0,3) (1,2)
// (1,3) (2,3); the columns of v become the eigenvectors, the diagonal of a the eigenvalues.
inline void jacobi4(double a[4][4], double v[4][4]) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
        for (int p = 0; p < 3; p++) {
            for (int q = p + 1; q < 4; q++) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                // tan of the rotation angle, the smaller root: t = sign(theta) / (|theta| + sqrt(theta^2 + 1))
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; k++) {      // a <- a J
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; k++) {      // a <- J^T a
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                a[p][q] = a[q][p] = 0.0;
                for (int k = 0; k < 4; k++) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
}

// the rotation matrix of the unit quaternion (w, x, y, z), row-major
inline void quat_matrix(const double q[4], double R[3][3]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z); R[0][1] = 2.0 * (x * y - w * z);       R[0][2] = 2.0 * (x * z + w * y);
    R[1][0] = 2.0 * (x * y + w * z);       R[1][1] = 1.0 - 2.0 * (x * x + z * z); R[1][2] = 2.0 * (y * z - w * x);
    R[2][0] = 2.0 * (x * z - w * y);       R[2][1] = 2.0 * (y * z + w * x);       R[2][2] = 1.0 - 2.0 * (x * x + y * y);
}

// Horn's closed form from the sums.  Returns null, or why the sums determine no transform (*delta_out, *rms_out untouched).
inline const char *rigid_fit(const gs_pair_sums *sums, int with_scale, gs_model_transform_pod *delta_out, double *rms_out) {
    if (sums->pairs < 3u) return "a rigid fit takes at least 3 pairs";
    bool finite = std::isfinite(sums->spp) && std::isfinite(sums->sqq) && std::isfinite(sums->sdd);
    for (int a = 0; a < 3; a++) finite = finite && std::isfinite(sums->sp[a]) && std::isfinite(sums->sq[a]);
    for (int a = 0; a < 9; a++) finite = finite && std::isfinite(sums->spq[a]);
    if (!finite) return "a sum is not finite";
    const double n = (double)sums->pairs;
    double pm[3], qm[3], H[3][3];
    for (int a = 0; a < 3; a++) {
        pm[a] = sums->sp[a] / n;
        qm[a] = sums->sq[a] / n;
    }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) H[a][b] = sums->spq[3 * a + b] - sums->sp[a] * sums->sq[b] / n;
    const double spread = sums->spp - ((sums->sp[0] * sums->sp[0] + sums->sp[1] * sums->sp[1]) + sums->sp[2] * sums->sp[2]) / n;
    if (!(spread > 0.0) || !std::isfinite(spread)) return "the query points of the pairs have no spread";
    // Horn 1987, the symmetric matrix whose largest eigenvector is the quaternion (w, x, y, z) of the rotation p -> q
    double N[4][4] = {
        {(H[0][0] + H[1][1]) + H[2][2], H[1][2] - H[2][1], H[2][0] - H[0][2], H[0][1] - H[1][0]},
        {H[1][2] - H[2][1], (H[0][0] - H[1][1]) - H[2][2], H[0][1] + H[1][0], H[2][0] + H[0][2]},
        {H[2][0] - H[0][2], H[0][1] + H[1][0], (H[1][1] - H[0][0]) - H[2][2], H[1][2] + H[2][1]},
        {H[0][1] - H[1][0], H[2][0] + H[0][2], H[1][2] + H[2][1], (H[2][2] - H[0][0]) - H[1][1]},
    };
    double fro = 0.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            if (!std::isfinite(N[i][j])) return "a sum is not finite";
            fro += N[i][j] * N[i][j];
        }
    fro = std::sqrt(fro);
    double V[4][4];
    jacobi4(N, V);
    int top = 0;
    for (int i = 1; i < 4; i++)
        if (N[i][i] > N[top][top]) top = i;
    double second = -INFINITY;
    for (int i = 0; i < 4; i++)
        if (i != top && N[i][i] > second) second = N[i][i];
    if (!(N[top][top] - second > GAP_MIN * fro)) return "the pairs do not determine a rotation (collinear or coincident points)";
    double q[4] = {V[0][top], V[1][top], V[2][top], V[3][top]};
    const double len = std::sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    // w >= 0; w = 0: the first component that is not zero is positive
    double sign = 1.0;
    for (int i = 0; i < 4; i++)
        if (q[i] != 0.0) {
            sign = q[i] < 0.0 ? -1.0 : 1.0;
            break;
        }
    for (int i = 0; i < 4; i++) q[i] = sign * q[i] / len;
    double R[3][3];
    quat_matrix(q, R);
    double scale = 1.0;
    if (with_scale) {      // sum q' . R p' / sum |p'|^2
        double num = 0.0;
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) num += R[a][b] * H[b][a];
        scale = num / spread;
        if (!(scale > 0.0) || !std::isfinite(scale)) return "the pairs do not determine a scale";
    }
    gs_model_transform_pod d;
    for (int a = 0; a < 3; a++) {
        d.pos[a] = (float)(qm[a] - scale * ((R[a][0] * pm[0] + R[a][1] * pm[1]) + R[a][2] * pm[2]));
        d.scale[a] = (float)scale;
    }
    d.rot[0] = (float)q[1];
    d.rot[1] = (float)q[2];
    d.rot[2] = (float)q[3];
    d.rot[3] = (float)q[0];
    d._pad0 = d._pad1 = 0.0f;
    *delta_out = d;
    if (rms_out) *rms_out = std::sqrt(sums->sdd / n);
    return nullptr;
}

// out = the pod of delta o m, delta of uniform scale delta->scale[0]: rot = r_d r (Hamilton product), scale = s_d scale,
// pos = s_d R_d pos + t_d, in binary64 and rounded once.  out may be delta or m.
inline void compose(const gs_model_transform_pod *delta, const gs_model_transform_pod *m, gs_model_transform_pod *out) {
    const double dq[4] = {(double)delta->rot[3], (double)delta->rot[0], (double)delta->rot[1], (double)delta->rot[2]};      // w x y z
    const double mq[4] = {(double)m->rot[3], (double)m->rot[0], (double)m->rot[1], (double)m->rot[2]};
    const double s = (double)delta->scale[0];
    double R[3][3];
    quat_matrix(dq, R);
    gs_model_transform_pod r;
    const double w = ((dq[0] * mq[0] - dq[1] * mq[1]) - dq[2] * mq[2]) - dq[3] * mq[3];
    const double x = ((dq[0] * mq[1] + dq[1] * mq[0]) + dq[2] * mq[3]) - dq[3] * mq[2];
    const double y = ((dq[0] * mq[2] - dq[1] * mq[3]) + dq[2] * mq[0]) + dq[3] * mq[1];
    const double z = ((dq[0] * mq[3] + dq[1] * mq[2]) - dq[2] * mq[1]) + dq[3] * mq[0];
    r.rot[0] = (float)x;
    r.rot[1] = (float)y;
    r.rot[2] = (float)z;
    r.rot[3] = (float)w;
    for (int a = 0; a < 3; a++) {
        r.pos[a] = (float)(s * ((R[a][0] * (double)m->pos[0] + R[a][1] * (double)m->pos[1]) + R[a][2] * (double)m->pos[2]) + (double)delta->pos[a]);
        r.scale[a] = (float)(s * (double)m->scale[a]);
    }
    r._pad0 = r._pad1 = 0.0f;
    *out = r;
}

}  // namespace gsfit
