/*
 * ll_pose_info.h -- from the 28 sums of ll_map_neq.h to an ll_pose_info record (include/lightloam_hip.h): H and g unpacked by
 * ll_neq_unpack, the residual variance from the fit record's plain squares, the eigenvalues of H.  One thread does all of it; both
 * k_cms_info (ll_localize.hip) and k_al_infosum (ll_map_align.hip) end here, so the two stages' records are made by one text.
 */
#pragma once
#include "ll_map_neq.h"

#define LL_INFO_SWEEPS 12                     /* cyclic Jacobi on a symmetric 6 x 6: converged to the last bit long before */

/* the eigenvalues of the symmetric a [6][6] (destroyed), ascending.  Every sweep visits (0,1) (0,2) .. (4,5); a pair whose off-diagonal
 * entry is exactly 0 is left alone.  A' = J^T A J with J = [c s ; -s c] in the (p, q) plane, t = tan of the angle that zeroes a_pq,
 * the smaller root.  The 15 rotations of a sweep are unrolled, so every index is a constant and the matrix stays in registers: the
 * one thread that runs this waits for its own square roots and divisions, not for memory */
__device__ __forceinline__ void ll_info_eig(double (&a)[36], double eig[6])
{
#pragma unroll 1
    for (int sweep = 0; sweep < LL_INFO_SWEEPS; ++sweep)
#pragma unroll
        for (int p = 0; p < 5; ++p)
#pragma unroll
            for (int q = p + 1; q < 6; ++q) {
                const double apq = a[p * 6 + q];
                if (apq == 0.0) continue;
                const double theta = (a[q * 6 + q] - a[p * 6 + p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const double akp = a[k * 6 + p], akq = a[k * 6 + q];
                    a[k * 6 + p] = c * akp - s * akq; a[k * 6 + q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const double apk = a[p * 6 + k], aqk = a[q * 6 + k];
                    a[p * 6 + k] = c * apk - s * aqk; a[q * 6 + k] = s * apk + c * aqk;
                }
            }
#pragma unroll
    for (int k = 0; k < 6; ++k) eig[k] = a[k * 7];
#pragma unroll
    for (int i = 1; i < 6; ++i)                                   /* a fixed network: every compare-exchange of a bubble sort */
#pragma unroll
        for (int k = 0; k < 6 - i; ++k) {
            const double lo = eig[k] <= eig[k + 1] ? eig[k] : eig[k + 1], hi = eig[k] <= eig[k + 1] ? eig[k + 1] : eig[k];
            eig[k] = lo; eig[k + 1] = hi;
        }
}

/* tot: the 28 sums; F: the fit record of the same blocks; work: 44 doubles of LDS.  One thread */
__device__ __forceinline__ void ll_info_finish(const double *tot, const ll_localize_fit &F, double *work, ll_pose_info *out)
{
    const int rows = 3 * F.n_edge + F.n_plane;
    double *neq = work, a[36];
    ll_neq_unpack(tot, rows, neq);
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 36; ++k) { out->H[k] = neq[k]; a[k] = neq[k]; finite = finite && (neq[k] - neq[k] == 0.0); }
    for (int k = 0; k < 6; ++k) out->g[k] = neq[36 + k];
    double eig[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (finite) ll_info_eig(a, eig);
#pragma unroll
    for (int k = 0; k < 6; ++k) out->eig[k] = eig[k];
    out->sigma2 = rows > 6 ? (F.sq_edge + F.sq_plane) / (double)(rows - 6) : 0.0;
    out->rows = rows;
    out->flags = (finite ? 0 : 1) | (rows <= 6 ? 2 : 0);
}
