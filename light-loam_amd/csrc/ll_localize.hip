/*
 * ll_localize.hip -- how well a localised pose fits the frozen map it was solved against (ll_cubemaps_localize_slots' fit record).
 * After the last k_cms_lm launch the residual blocks of every view are rebuilt at the final pose (k_cms_knn + k_cms_compact,
 * ll_cubemaps.hip); k_cms_fit then reduces them: the block counts, the Huber cost ll_map_normal_equations reports there and the
 * plain sums of squares of the edge and the plane residuals.  Nothing here changes a pose or a map.
 */
#include "ll_cubemap.h"
#include "ll_factor_math.h"

#define LL_FIT_NACC 3     /* cost, sq_edge, sq_plane */

/* one workgroup per view: the rows of k_map_normal_eq without the Jacobians' products, summed in f64 -- per thread, then over the
 * wave, then over the four waves through LDS in wave order.  The record of view v goes to fit[(views[v].pose - pose0) / 7], the
 * sequence the view's pose row belongs to, with plain stores by thread 0. */
__global__ __launch_bounds__(256) void k_cms_fit(const LLMapView *views, const double *pose0, ll_localize_fit *fit)
{
    const LLMapView &M = views[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_e = M.counts[0], n_p = M.counts[1];
    Pose P;
    for (int k = 0; k < 4; ++k) P.q[k] = M.pose[k];
    for (int k = 0; k < 3; ++k) P.t[k] = M.pose[4 + k];
    double acc[LL_FIT_NACC] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n_e; i += 256) {
        double r[3], Jq[3][4], Jt[3][3];
        ll_edge_d(P, M.stk[0][M.src[0][i]], &M.fa[(size_t)i * 3], &M.fb[(size_t)i * 3], r, Jq, Jt);
        const double sq = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        (void)ll_huber_scale(sq, M.huber, acc[0]);
        acc[1] += sq;
    }
    for (int i = tid; i < n_p; i += 256) {
        double r, Jq[4], Jt[3];
        ll_plane_norm(P, M.stk[1][M.src[1][i]], &M.fn[(size_t)i * 3], M.fd[i], r, Jq, Jt);
        (void)ll_huber_scale(r * r, M.huber, acc[0]);
        acc[2] += r * r;
    }
    __shared__ double red[4][LL_FIT_NACC];
#pragma unroll
    for (int k = 0; k < LL_FIT_NACC; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        ll_localize_fit F;
        F.n_edge = n_e; F.n_plane = n_p;
        F.cost = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        F.sq_edge = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        F.sq_plane = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
        fit[(M.pose - pose0) / 7] = F;
    }
}

void ll_launch_cms_fit(const LLMapView *d_views, int n_views, const double *d_pose0, ll_localize_fit *d_fit, hipStream_t st)
{
    if (n_views > 0) hipLaunchKernelGGL(k_cms_fit, dim3((unsigned)n_views), dim3(256), 0, st, d_views, d_pose0, d_fit);
}
