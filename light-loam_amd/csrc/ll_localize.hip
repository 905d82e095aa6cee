/*
 * ll_localize.hip -- how well a localised pose fits the frozen map it was solved against (ll_cubemaps_localize_slots' fit record).
 * After the last k_cms_lm launch the residual blocks of every view are rebuilt at the final pose (k_cms_knn + k_cms_compact,
 * ll_cubemaps.hip); k_cms_fit then reduces them: the block counts, the Huber cost ll_map_normal_equations reports there and the
 * plain sums of squares of the edge and the plane residuals.  k_cms_info reduces the same blocks once more into the information
 * record (ll_pose_info: the normal equations' H and g there, their eigenvalues, the residual variance).  Nothing here changes a pose or a map.
 */
#include "ll_cubemaps.h"
#include "ll_map_neq.h"
#include "ll_pose_info.h"

/* one workgroup per view: the blocks of k_map_normal_eq without the Jacobians' products (ll_map_fit_edge / _plane, ll_map_neq.h),
 * summed in f64 -- per thread, then over the wave, then over the four waves through LDS in wave order.  The record of view v goes
 * to fit[(views[v].pose - pose0) / 7], the sequence the view's pose row belongs to, with plain stores by thread 0. */
__global__ __launch_bounds__(256) void k_cms_fit(const LLMapView *views, const double *pose0, ll_localize_fit *fit)
{
    const LLMapView &M = views[blockIdx.x];
    const int tid = threadIdx.x;
    const Pose P = ll_pose_load(M.pose);
    double acc[LL_FIT_NACC] = {0.0, 0.0, 0.0};                    /* cost, sq_edge, sq_plane */
    ll_map_acc_blocks(M, P, tid, 256, acc);
    __shared__ double red[4][LL_FIT_NACC];
    ll_wg_sum<LL_FIT_NACC>(acc, red);
    if (tid == 0) {
        ll_localize_fit F;
        F.n_edge = M.counts[0]; F.n_plane = M.counts[1];
        F.cost = ll_wg_total(red, 0); F.sq_edge = ll_wg_total(red, 1); F.sq_plane = ll_wg_total(red, 2);
        fit[(M.pose - pose0) / 7] = F;
    }
}

void ll_launch_cms_fit(const LLMapView *d_views, int n_views, const double *d_pose0, ll_localize_fit *d_fit, hipStream_t st)
{
    if (n_views > 0) hipLaunchKernelGGL(k_cms_fit, dim3((unsigned)n_views), dim3(256), 0, st, d_views, d_pose0, d_fit);
}

/* one workgroup per view: k_map_normal_eq's 28 sums over the same blocks (ll_map_acc_edge / _plane), reduced like k_cms_fit, then
 * thread 0 makes the ll_pose_info record (ll_pose_info.h) with the squares k_cms_fit left in fit[] -- launched behind it */
__global__ __launch_bounds__(256) void k_cms_info(const LLMapView *views, const double *pose0, const ll_localize_fit *fit, ll_pose_info *info)
{
    const LLMapView &M = views[blockIdx.x];
    const int tid = threadIdx.x;
    const Pose P = ll_pose_load(M.pose);
    double acc[LL_NACC];
#pragma unroll
    for (int k = 0; k < LL_NACC; ++k) acc[k] = 0.0;
    ll_map_acc_blocks(M, P, tid, 256, acc);
    __shared__ double red[4][LL_NACC], stot[LL_NACC], work[LL_NEQ_STRIDE];
    ll_wg_sum<LL_NACC>(acc, red);
    if (tid < LL_NACC) stot[tid] = ll_wg_total(red, tid);
    __syncthreads();
    if (tid == 0) {
        const size_t q = (size_t)((M.pose - pose0) / 7);
        ll_info_finish(stot, fit[q], work, info + q);
    }
}

void ll_launch_cms_info(const LLMapView *d_views, int n_views, const double *d_pose0, const ll_localize_fit *d_fit, ll_pose_info *d_info, hipStream_t st)
{
    if (n_views > 0) hipLaunchKernelGGL(k_cms_info, dim3((unsigned)n_views), dim3(256), 0, st, d_views, d_pose0, d_fit, d_info);
}
