/*
 * ll_map_neq.h -- the ONE definition of laserMapping's normal equations: what a residual block adds to the 28 sums (or to the
 * three sums of a fit record), the workgroup reduction behind them, the order of the partial sums, the 44-double record and one
 * round of the trust-region solve on it.  The library is built with -ffp-contract=off: the operation order written here IS the
 * result, so the kernels that call these functions -- k_map_normal_eq, k_map_lm_solve (ll_mapping.hip), k_cms_lm (ll_cubemaps.hip),
 * k_cms_fit / k_cms_info (ll_localize.hip), k_al_eval / k_al_solve / k_al_fitsum / k_al_infosum (ll_map_align.hip) -- agree bit for bit because they share
 * this text, not because copies were kept alike.  What stays in a kernel is mechanism: which blocks a thread takes, how partial sums
 * travel between workgroups, when a round begins.  ll_neq_eval (ll_neq.h: the odometry's blocks, on the flagship path) keeps its own
 * text of the reduction and the record: sharing them re-schedules k_normal_equations / k_lm_solve / k_vote_lm_rows (ll_sequences.hip).
 * Every function is force-inlined and takes the accumulators as a reference to the caller's array: they stay in registers.
 */
#pragma once
#include "ll_common.h"
#include "ll_factor_math.h"
#include "ll_lm_step.h"

__device__ __forceinline__ Pose ll_pose_load(const double *p7)
{
    Pose P;
    for (int k = 0; k < 4; ++k) P.q[k] = p7[k];
    for (int k = 0; k < 3; ++k) P.t[k] = p7[4 + k];
    return P;
}

/* ---- one residual block: LidarEdgeFactor (3 rows) / LidarPlaneNormFactor (1 row), HuberLoss, EigenQuaternionManifold ---- */
__device__ __forceinline__ void ll_map_acc_edge(const LLMapView &M, const Pose &P, int i, double (&acc)[LL_NACC])
{
    double r[3], Jq[3][4], Jt[3][3];
    ll_edge_d(P, M.stk[0][M.src[0][i]], &M.fa[(size_t)i * 3], &M.fb[(size_t)i * 3], r, Jq, Jt);
    const double sc = ll_huber_scale(r[0] * r[0] + r[1] * r[1] + r[2] * r[2], M.huber, acc[27]);
    for (int row = 0; row < 3; ++row) {
        double J[6];
        ll_to_local(P, Jq[row], J);
        J[3] = Jt[row][0]; J[4] = Jt[row][1]; J[5] = Jt[row][2];
        for (int k = 0; k < 6; ++k) J[k] *= sc;
        ll_acc_row(acc, J, r[row] * sc);
    }
}
__device__ __forceinline__ void ll_map_acc_plane(const LLMapView &M, const Pose &P, int i, double (&acc)[LL_NACC])
{
    double r, Jq[4], Jt[3], J[6];
    ll_plane_norm(P, M.stk[1][M.src[1][i]], &M.fn[(size_t)i * 3], M.fd[i], r, Jq, Jt);
    const double sc = ll_huber_scale(r * r, M.huber, acc[27]);
    ll_to_local(P, Jq, J);
    J[3] = Jt[0]; J[4] = Jt[1]; J[5] = Jt[2];
    for (int k = 0; k < 6; ++k) J[k] *= sc;
    ll_acc_row(acc, J, r * sc);
}

/* the same blocks without the Jacobians' products: acc[0] += the Huber cost, acc[1] / acc[2] += the plain squares (ll_localize_fit) */
#define LL_FIT_NACC 3
template <int N>
__device__ __forceinline__ void ll_map_fit_edge(const LLMapView &M, const Pose &P, int i, double (&acc)[N])
{
    double r[3], Jq[3][4], Jt[3][3];
    ll_edge_d(P, M.stk[0][M.src[0][i]], &M.fa[(size_t)i * 3], &M.fb[(size_t)i * 3], r, Jq, Jt);
    const double sq = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    (void)ll_huber_scale(sq, M.huber, acc[0]);
    acc[1] += sq;
}
template <int N>
__device__ __forceinline__ void ll_map_fit_plane(const LLMapView &M, const Pose &P, int i, double (&acc)[N])
{
    double r, Jq[4], Jt[3];
    ll_plane_norm(P, M.stk[1][M.src[1][i]], &M.fn[(size_t)i * 3], M.fd[i], r, Jq, Jt);
    (void)ll_huber_scale(r * r, M.huber, acc[0]);
    acc[2] += r * r;
}

/* blocks first, first + stride, ... : the edges, then the planes.  An LL_NACC-wide acc takes the normal equations, an
 * LL_FIT_NACC-wide one the fit sums */
__device__ __forceinline__ void ll_map_acc_blocks(const LLMapView &M, const Pose &P, int first, int stride, double (&acc)[LL_NACC])
{
    const int n_e = M.counts[0], n_p = M.counts[1];
    for (int i = first; i < n_e; i += stride) ll_map_acc_edge(M, P, i, acc);
    for (int i = first; i < n_p; i += stride) ll_map_acc_plane(M, P, i, acc);
}
__device__ __forceinline__ void ll_map_acc_blocks(const LLMapView &M, const Pose &P, int first, int stride, double (&acc)[LL_FIT_NACC])
{
    const int n_e = M.counts[0], n_p = M.counts[1];
    for (int i = first; i < n_e; i += stride) ll_map_fit_edge(M, P, i, acc);
    for (int i = first; i < n_p; i += stride) ll_map_fit_plane(M, P, i, acc);
}

/* ---- the sums of a workgroup: over the wave by shuffles, lane 0 of wave w leaves red[w][k], then a barrier ---- */
template <int N, int NA, int NR>
__device__ __forceinline__ void ll_wg_sum(const double (&acc)[NA], double (*red)[NR])
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
}
/* sum k of a 256-thread workgroup: its four waves, left to right */
template <int NR>
__device__ __forceinline__ double ll_wg_total(double (*red)[NR], int k)
{
    return ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}
/* sum k of n partial sums [n][LL_NACC], in workgroup (or chunk) order */
__device__ __forceinline__ double ll_partials_sum(const double *spart, int n, int k)
{
    double v = 0.0;
    for (int b = 0; b < n; ++b) v += spart[(size_t)b * LL_NACC + k];
    return v;
}

/* the 28 sums -> the 44-double record: H [6][6] from its upper triangle, g [6], cost, rows */
__device__ __forceinline__ void ll_neq_unpack(const double *tot, int rows, double *out)
{
    int k = 0;
    for (int a = 0; a < 6; ++a) for (int b = a; b < 6; ++b) { out[a * 6 + b] = tot[k]; out[b * 6 + a] = tot[k]; ++k; }
    for (int a = 0; a < 6; ++a) out[36 + a] = tot[21 + a];
    out[42] = tot[27];
    out[43] = (double)rows;
}

/* round `round` of one ceres::Solve on one thread: sneq = the normal equations at the pose sp.  Round 0 begins the solve, a
 * later one accepts or rejects the step that led to sp; unless it is the last, sp becomes the next pose to evaluate */
__device__ __forceinline__ void ll_lm_round(double *sL, const double *sneq, double *sp, const LLLmOpt &o, int round)
{
    if (round == 0) ll_lm_begin_one(sL, sneq, sp, o); else ll_lm_accept_one(sL, sneq, sp, o);
    if (round < o.max_num_iterations) ll_lm_propose_one(sL, sp, o);
}
