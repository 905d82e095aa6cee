/*
 * ll_neq.h -- the normal equations of one slot by one workgroup (ll_neq_eval), shared by the solves of ll_factors.hip and the fused
 * vote + solve of ll_odometry_sequences (ll_sequences.hip).
 */
#pragma once
#include "ll_common.h"
#include "ll_factor_math.h"

/* the normal equations of slot s at the pose pose_in[7] (global or LDS), by the whole workgroup; thread 0 leaves the 44-double
 * record in out[] (global or LDS).  Ends with every thread past the last barrier but WITHOUT a barrier after thread 0's
 * stores: the caller synchronises before anybody else reads out[]. */
/* DIST: DISTORTION 1 (ll_params.distortion): a second instantiation of the kernels, so that the reference's own build (s = 1 everywhere) pays
 * neither a branch nor a register for it */
template <int NT, bool DIST>
__device__ __forceinline__ void ll_neq_eval(const LLView &V, int s, const double *pose_in, double *out, double (*red)[LL_NACC])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const PairHdr ph = V.pair[s];
    Pose P;
    for (int k = 0; k < 4; ++k) P.q[k] = pose_in[k];
    for (int k = 0; k < 3; ++k) P.t[k] = pose_in[4 + k];
    const float4 *corner, *surf; int mc, ms;
    ll_targets(V, s, corner, mc, surf, ms);
    const float4 *sharp = V.sharp + (size_t)s * V.cap_sharp, *flat = V.flat + (size_t)s * V.cap_flat;
    const int *es = V.e_src + (size_t)s * V.cap_sharp, *ea = V.e_a + (size_t)s * V.cap_sharp, *eb = V.e_b + (size_t)s * V.cap_sharp;
    const int *ps = V.p_src + (size_t)s * V.cap_flat, *pa = V.p_a + (size_t)s * V.cap_flat, *pb = V.p_b + (size_t)s * V.cap_flat, *pc = V.p_c + (size_t)s * V.cap_flat;
    const uint8_t *vs = V.v_sel + (size_t)s * V.cap_flat; const float *vw = V.v_w + (size_t)s * V.cap_flat;

    double acc[LL_NACC];
#pragma unroll
    for (int k = 0; k < LL_NACC; ++k) acc[k] = 0.0;
    for (int i = tid; i < ph.n_edge; i += NT) {
        double r[3], Jq[3][4], Jt[3][3];
        ll_edge(P, sharp[es[i]], corner[ea[i]], corner[eb[i]], r, Jq, Jt, DIST ? ll_point_s(1, sharp[es[i]]) : 1.0);
        const double sc = ll_huber_scale(r[0] * r[0] + r[1] * r[1] + r[2] * r[2], V.huber, acc[27]);
        for (int row = 0; row < 3; ++row) {
            double J[6];
            ll_to_local(P, Jq[row], J);
            J[3] = Jt[row][0]; J[4] = Jt[row][1]; J[5] = Jt[row][2];
            for (int k = 0; k < 6; ++k) J[k] *= sc;
            ll_acc_row(acc, J, r[row] * sc);
        }
    }
    for (int i = tid; i < ph.n_plane; i += NT) {
        if (!vs[i]) continue;
        double r, Jq[4], Jt[3], J[6];
        ll_plane(P, flat[ps[i]], surf[pa[i]], surf[pb[i]], surf[pc[i]], (double)vw[i], r, Jq, Jt, DIST ? ll_point_s(1, flat[ps[i]]) : 1.0);
        const double sc = ll_huber_scale(r * r, V.huber, acc[27]);
        ll_to_local(P, Jq, J);
        J[3] = Jt[0]; J[4] = Jt[1]; J[5] = Jt[2];
        for (int k = 0; k < 6; ++k) J[k] *= sc;
        ll_acc_row(acc, J, r * sc);
    }
#pragma unroll
    for (int k = 0; k < LL_NACC; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double tot[LL_NACC];
        for (int k = 0; k < LL_NACC; ++k) { double v = 0.0; for (int w = 0; w < NT / 64; ++w) v += red[w][k]; tot[k] = v; }
        int k = 0;
        for (int a = 0; a < 6; ++a) for (int b = a; b < 6; ++b) { out[a * 6 + b] = tot[k]; out[b * 6 + a] = tot[k]; ++k; }
        for (int a = 0; a < 6; ++a) out[36 + a] = tot[21 + a];
        out[42] = tot[27];
        out[43] = (double)(3 * ph.n_edge + ph.n_plane_sel);
    }
}

#define LL_LM_THREADS 512     /* the solve is a chain of 1 + max_num_iterations evaluations on ONE workgroup: twice the threads, half the chain */
