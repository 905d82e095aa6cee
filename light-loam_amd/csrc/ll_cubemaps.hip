/*
 * ll_cubemaps.hip -- laserMapping's per-frame body (laserMapping.cpp:1584-2165) for S cube maps side by side.
 * Sequence q is an ll_cubemap (ll_cubemap.h) whose pools are the q-th region of shared allocations and whose ll_map is its own;
 * its pair tables, centre and pool tops are host state exactly as for one cube map.  Frame k of every running sequence goes
 * through one set of launches per stage, and the host synchronises a fixed number of times per frame, whatever S is:
 *   slots      the scan headers of the running slots (ll_cubemaps_process_slots only)
 *   prepare    shift loops and valid cubes on the host; ONE k_cms_copy gathers every sequence's valid cubes and scans, one
 *              ll_voxel_grid_segments call per cloud type down-sizes every scan (a segment per sequence), k_cms_bbox boxes every
 *              search cloud; then the boxes and the stack sizes of all sequences come back together
 *   optimize   :1822 gate per sequence; 2 x {k_cms_knn (ll_map_knn_one per stack point over a block table of (sequence, cloud
 *              type, first point)), k_cms_compact (one workgroup per sequence and type), k_cms_lm (one workgroup per sequence
 *              for the whole ceres::Solve, the arithmetic of ll_map_neq.h)}; all poses come back once
 *   update     k_cms_assign (cm_assign_one, ll_cubemap.h, over a block table), a stable sort by cube per sequence, then the per-cube
 *              counts of all sequences; one ll_voxel_grid_segments call per type over every valid cube of every sequence,
 *              then the filtered sizes; the capacity decision for all sequences, the commit, one k_cms_copy for all clouds.
 * No kernel here waits on another workgroup.  k_cms_lm runs k_map_lm_solve's LL_NEQ_NB x 256-thread partition of the blocks as
 * LL_NEQ_NB passes of one 256-thread workgroup; block sums, reduction tree and the order of the partials are the same functions
 * of ll_map_neq.h in both: the normal equations, and so the poses, are bit for bit those of ll_cubemap_process_slot.  The grids of the search clouds
 * are still built per sequence (ll_map_rebuild_finish: a handful of launches each, no synchronisation).
 * ll_cubemaps_localize_slots is the same frame read-only: slots, prepare without the shift loops (the map may be another
 * sequence's and shared: cms_localize), optimize, no update -- three synchronisations; with a fit record, one more knn + compact
 * pass at the final poses and k_cms_fit (ll_localize.hip) before the poses' copy, which then carries the records too.
 */
#include "ll_cubemaps.h"
#include "ll_factor_math.h"
#include "ll_map_neq.h"
#include "ll_map_search.h"
#include <chrono>
#include <cmath>
#include <numeric>

/* dst[i] = index ? src[index[i]] : src[i], i < cnt */
struct CmsCopy { const float4 *src; const int *index; float4 *dst; int cnt, pad; };
/* one bounding box: 6 ordered ints (min xyz, max xyz) of pts[0, n) */
struct CmsBox { const float4 *pts; int *out; int n, pad; };
/* cm_assign_one's arguments for one (sequence, cloud type) */
struct CmsAssign { const float4 *stk; const double *pose; float4 *tp; unsigned long long *keys; int *vals; int *addcnt; int n, cen[3]; };

/* ------------------------------------------------------------------ kernels */
__global__ __launch_bounds__(256) void k_cms_copy(const CmsCopy *ops, int per)
{
    const CmsCopy op = ops[blockIdx.x / per];
    for (int i = (blockIdx.x % per) * 256 + threadIdx.x; i < op.cnt; i += per * 256) op.dst[i] = op.index ? op.src[op.index[i]] : op.src[i];
}

/* k_map_bbox for many clouds: one workgroup per cloud, no atomics (min / max do not depend on the order) */
__global__ __launch_bounds__(256) void k_cms_bbox(const CmsBox *boxes)
{
    const CmsBox B = boxes[blockIdx.x];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < B.n; i += 256) {
        const float4 p = B.pts[i];
        mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
    }
    for (int o = 32; o > 0; o >>= 1)
        for (int k = 0; k < 3; ++k) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o)); }
    __shared__ float red[4][6];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) for (int k = 0; k < 3; ++k) { red[wave][k] = mn[k]; red[wave][3 + k] = mx[k]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = red[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) v = threadIdx.x < 3 ? fminf(v, red[w][threadIdx.x]) : fmaxf(v, red[w][threadIdx.x]);
        B.out[threadIdx.x] = ll_f2ord(v);
    }
}

/* the search + fit of k_map_knn; block b covers the LL_KNNB stack points from blk[b].z of cloud type blk[b].y of view blk[b].x */
__global__ __launch_bounds__(LL_KNNB) void k_cms_knn(const LLMapView *views, const int4 *blk)
{
    const int4 b = blk[blockIdx.x];
    const LLMapView &M = views[b.x];
    if (b.y == 0) ll_map_knn_one<true>(M, b.z + threadIdx.x);
    else ll_map_knn_one<false>(M, b.z + threadIdx.x);
}

/* k_map_compact's result (residual blocks in stack order) for one (view, cloud type) per workgroup, chunk after chunk */
__global__ __launch_bounds__(256) void k_cms_compact(const LLMapView *views)
{
    __shared__ int sc[4];
    const LLMapView &M = views[blockIdx.x >> 1];
    const int which = blockIdx.x & 1, tid = threadIdx.x;
    const int n = M.n_stk[which];
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        const bool ok = i < n && M.ok[which][i];
        int total;
        const int pos = base + ll_block_exscan_n<4>(ok ? 1 : 0, sc, total);
        if (ok) ll_map_place(M, which, pos, i);
        base += total;
    }
    if (tid == 0) M.counts[which] = base;
}

/* one ceres::Solve per view on one workgroup: k_map_lm_solve's rounds, its LL_NEQ_NB workgroups' partial sums taken as
 * LL_NEQ_NB passes (thread tid of pass b does what thread tid of workgroup b does), summed in workgroup order */
__global__ __launch_bounds__(256) void k_cms_lm(const LLMapView *views, LLLmOpt o)
{
    const LLMapView &M = views[blockIdx.x];
    const int tid = threadIdx.x, gsz = LL_NEQ_NB * 256;
    const int n_e = M.counts[0], n_p = M.counts[1];
    __shared__ double red[4][LL_NACC];
    __shared__ double sp[7], sneq[LL_NEQ_STRIDE], sL[LL_LM_STRIDE], stot[LL_NACC], spart[LL_NEQ_NB * LL_NACC];
    for (int k = tid; k < LL_LM_STRIDE; k += 256) sL[k] = 0.0;
    if (tid < 7) sp[tid] = M.pose[tid];
    __syncthreads();
    for (int round = 0; round <= o.max_num_iterations; ++round) {
        const Pose P = ll_pose_load(sp);
        for (int wg = 0; wg < LL_NEQ_NB; ++wg) {
            double acc[LL_NACC];
#pragma unroll
            for (int k = 0; k < LL_NACC; ++k) acc[k] = 0.0;
            ll_map_acc_blocks(M, P, wg * 256 + tid, gsz, acc);
            ll_wg_sum<LL_NACC>(acc, red);
            if (tid < LL_NACC) spart[wg * LL_NACC + tid] = ll_wg_total(red, tid);
            __syncthreads();
        }
        if (tid < LL_NACC) stot[tid] = ll_partials_sum(spart, LL_NEQ_NB, tid);
        __syncthreads();
        if (tid == 0) {
            ll_neq_unpack(stot, 3 * n_e + n_p, sneq);
            ll_lm_round(sL, sneq, sp, o, round);
        }
        __syncthreads();
    }
    if (tid < 7) M.pose[tid] = sp[tid];
    for (int k = tid; k < LL_NEQ_STRIDE; k += 256) M.neq[k] = sneq[k];
    for (int k = tid; k < LL_LM_STRIDE; k += 256) M.lm[k] = sL[k];
}

/* cm_assign_one (ll_cubemap.h; one cube map each, no tile shard) for the 256 stack points from blk[b].y of record blk[b].x */
__global__ __launch_bounds__(256) void k_cms_assign(const CmsAssign *recs, const int2 *blk)
{
    const int2 b = blk[blockIdx.x];
    const CmsAssign &A = recs[b.x];
    cm_assign_one(A.stk, A.n, A.pose, A.cen, 0, 1, A.tp, A.keys, A.vals, A.addcnt, b.y + threadIdx.x);
}

/* ------------------------------------------------------------------ host side */
/* the per-call tables go up through page-locked memory: arena `par` of a call is written only after the call before the previous
 * one has synchronised, so no copy of it can still be in flight; a table that does not fit moves to a larger arena (the old one
 * is kept until destroy: copies and kernels of this call may still read it) */
static_assert(sizeof(ll_localize_fit) == 4 * sizeof(double), "the fit records lie behind the poses as 4 doubles each");
static_assert(sizeof(ll_pose_info) == 50 * sizeof(double), "the information records lie behind the fit records as 50 doubles each");
struct CmsArena { unsigned char *h = nullptr, *d = nullptr; size_t cap = 0, used = 0; };

struct ll_cubemaps {
    ll_ctx *ctx = nullptr;
    int S = 0;
    float leaf[2] = {0.4f, 0.8f};
    int cap_last[2] = {0, 0}, cap_work = 0;
    size_t cap_pool = 0;
    std::vector<ll_cubemap *> cm;                 /* sequence q: pools = region q of pool_mem, its own ll_map */
    float4 *pool_mem[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    float4 *d_last[2] = {nullptr, nullptr}, *d_stk_out[2] = {nullptr, nullptr}, *d_tp[2] = {nullptr, nullptr};   /* [S][cap_last[w]] */
    unsigned long long *d_keys[2] = {nullptr, nullptr}; int *d_vals[2] = {nullptr, nullptr};
    float4 *d_work[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};                                   /* [S][cap_work] */
    int *d_addcnt = nullptr, *d_nout = nullptr, *d_bbox = nullptr;
    double *d_pose = nullptr;                     /* [S][7]: the pose every stage of a frame reads */
    ll_localize_fit *d_fit = nullptr;             /* [S], right behind d_pose: one copy brings both to the host */
    ll_pose_info *d_info = nullptr;               /* [S], right behind d_fit: the same copy brings them too */
    LLVoxWork W[2], WS;                           /* per cloud type: prepare's and update's filters; WS: the by-cube sort */
    CmsArena ar[2]; int par = 0;
    LLMapExport X;                                /* ll_cubemaps_export's staging buffer and events */
    LLMapMerge G;                                 /* ll_cubemaps_merge's workspace and events */
    LLMapAlign A;                                 /* ll_cubemaps_align's workspace and events */
    std::vector<void *> allocs, host_allocs;
    long long syncs = 0, frames = 0;
    std::string err;
};

#define CMS_HIP(call) LL_HIP_CHECK(ll_fail, cms, "", call, #call)

template <typename T>
static bool cms_alloc(ll_cubemaps *cms, T *&ptr, size_t count) { return ll_dev_alloc(cms->allocs, cms->err, ptr, count, false); }

/* host bytes -> device: through the call's page-locked arena; dst == nullptr: into the arena's device half (returned) */
static void *cms_stage(ll_cubemaps *cms, const void *src, size_t bytes, void *dst = nullptr)
{
    CmsArena &A = cms->ar[cms->par];
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (A.used + need > A.cap) {
        const size_t cap = std::max<size_t>(std::max<size_t>(2 * A.cap, need), (size_t)1 << 20);
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, cap, hipHostMallocDefault) != hipSuccess) { cms->err = "hipHostMalloc failed"; return nullptr; }
        cms->host_allocs.push_back(h);
        if (hipMalloc(&d, cap) != hipSuccess) { cms->err = "hipMalloc failed"; return nullptr; }
        cms->allocs.push_back(d);
        A.h = (unsigned char *)h; A.d = (unsigned char *)d; A.cap = cap; A.used = 0;
    }
    unsigned char *h = A.h + A.used, *d = A.d + A.used;
    A.used += need;
    if (bytes) std::memcpy(h, src, bytes);
    if (!dst) dst = d;
    if (bytes && hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, cms->ctx->stream) != hipSuccess) { cms->err = "upload failed"; return nullptr; }
    return dst;
}

/* device -> the arena's host half, then one synchronisation; returns the host copy */
static int cms_sync(ll_cubemaps *cms)
{
    CMS_HIP(hipStreamSynchronize(cms->ctx->stream));
    ++cms->syncs;
    return LL_OK;
}

static int cms_copy(ll_cubemaps *cms, const std::vector<CmsCopy> &ops)
{
    if (ops.empty()) return LL_OK;
    int mx = 1;
    for (const CmsCopy &o : ops) mx = std::max(mx, o.cnt);
    const CmsCopy *d = (const CmsCopy *)cms_stage(cms, ops.data(), ops.size() * sizeof(CmsCopy));
    if (!d) return LL_ERR_HIP;
    const int per = std::min(64, (mx + 255) / 256);
    hipLaunchKernelGGL(k_cms_copy, dim3((unsigned)(ops.size() * per)), dim3(256), 0, cms->ctx->stream, d, per);
    return LL_OK;
}

/* the voxel filter's sort reads back once when it cannot stay inside the workgroups (ll_voxel.hip): counted with the syncs */
static int cms_voxel(ll_cubemaps *cms, int w, const float4 *pts, const std::vector<int> &seg_off, float4 *out, int *n_out_dev)
{
    const int nseg = (int)seg_off.size() - 1, n = seg_off.back(), max_seg = nseg > 1 ? cm_max_segment(seg_off) : 0;
    if (!cms_stage(cms, seg_off.data(), seg_off.size() * sizeof(int), cms->W[w].seg_off)) return LL_ERR_HIP;
    if (ll_voxel_grid_segments_reads_back(n, nseg, max_seg)) ++cms->syncs;
    if (ll_voxel_grid_segments(pts, n, nseg, cms->leaf[w], cms->W[w], out, n_out_dev, cms->ctx->stream, max_seg)) { cms->err = "voxel filter: read-back failed"; return LL_ERR_HIP; }
    return LL_OK;
}

extern "C" void ll_cubemaps_destroy(ll_cubemaps *cms)
{
    if (!cms) return;
    if (cms->ctx) { (void)hipSetDevice(cms->ctx->device); (void)hipStreamSynchronize(cms->ctx->stream); }
    for (ll_cubemap *cm : cms->cm) ll_cubemap_destroy(cm);
    for (void *p : cms->allocs) (void)hipFree(p);
    for (void *p : cms->host_allocs) (void)hipHostFree(p);
    llx_free(cms->X);
    llmm_free(cms->G);
    llal_free(cms->A);
    delete cms;
}

extern "C" const char *ll_cubemaps_last_error(const ll_cubemaps *cms) { return cms ? cms->err.c_str() : "null cube maps"; }

extern "C" int ll_cubemaps_create(ll_ctx *ctx, int n_seq, float line_res, float plane_res, int max_scan_corner, int max_scan_surf, int pool_points, ll_cubemaps **out)
{
    if (!ctx || !out) return LL_ERR_ARG;
    *out = nullptr;
    if (n_seq < 1 || n_seq > 4096 || !(line_res > 0.0f) || !(plane_res > 0.0f) || max_scan_corner < 1 || max_scan_surf < 1 || pool_points < 4096 || pool_points > (1 << 26)) {
        ctx->err = "bad cube maps parameters"; return LL_ERR_ARG;
    }
    const int cap_from_map = std::min(pool_points, 1 << 24), mx_last = std::max(max_scan_corner, max_scan_surf);
    if (cap_from_map < mx_last) { ctx->err = "pool_points must be at least the scan capacity"; return LL_ERR_ARG; }
    if ((size_t)n_seq * (size_t)cap_from_map > (size_t)(INT_MAX / 2)) { ctx->err = "n_seq x pool_points too large for one filter call"; return LL_ERR_ARG; }
    LL_HIP(hipSetDevice(ctx->device));
    ll_cubemaps *cms = new ll_cubemaps();
    cms->ctx = ctx; cms->S = n_seq;
    cms->leaf[0] = line_res; cms->leaf[1] = plane_res;
    cms->cap_last[0] = max_scan_corner; cms->cap_last[1] = max_scan_surf;
    cms->cap_pool = (size_t)pool_points; cms->cap_work = cap_from_map;
    const size_t S = (size_t)n_seq;
    bool ok = true;
    for (int w = 0; w < 2 && ok; ++w) {
        ok = ok && cms_alloc(cms, cms->pool_mem[w][0], S * cms->cap_pool) && cms_alloc(cms, cms->pool_mem[w][1], S * cms->cap_pool);
        ok = ok && cms_alloc(cms, cms->d_last[w], S * cms->cap_last[w]) && cms_alloc(cms, cms->d_stk_out[w], S * cms->cap_last[w]) &&
             cms_alloc(cms, cms->d_tp[w], S * cms->cap_last[w]) && cms_alloc(cms, cms->d_keys[w], S * cms->cap_last[w]) &&
             cms_alloc(cms, cms->d_vals[w], S * cms->cap_last[w]);
        ok = ok && cms_alloc(cms, cms->d_work[w], S * cap_from_map) && cms_alloc(cms, cms->d_out[w], S * cap_from_map);
    }
    ok = ok && cms_alloc(cms, cms->d_addcnt, S * 2 * (CM_N + 1)) && cms_alloc(cms, cms->d_nout, 4) && cms_alloc(cms, cms->d_bbox, S * 12) &&
         cms_alloc(cms, cms->d_pose, S * 7 + S * (sizeof(ll_localize_fit) / sizeof(double)) + S * (sizeof(ll_pose_info) / sizeof(double)));
    if (ok) { cms->d_fit = (ll_localize_fit *)(cms->d_pose + S * 7); cms->d_info = (ll_pose_info *)(cms->d_fit + S); }
    for (int w = 0; w < 2 && ok; ++w) {
        unsigned char *p = nullptr;
        ok = cms_alloc(cms, p, ll_vox_work_bytes((int)(S * cap_from_map), (int)(S * 125)));
        if (ok) ll_vox_work_carve(p, (int)(S * cap_from_map), (int)(S * 125), &cms->W[w]);
    }
    if (ok) {
        unsigned char *p = nullptr;
        ok = cms_alloc(cms, p, ll_vox_work_bytes(mx_last, 1));
        if (ok) ll_vox_work_carve(p, mx_last, 1, &cms->WS);
    }
    for (int q = 0; q < n_seq && ok; ++q) {
        ll_cubemap *cm = new ll_cubemap();
        cms->cm.push_back(cm);
        cm->ctx = ctx;
        cm->leaf[0] = line_res; cm->leaf[1] = plane_res;
        cm->cap_last[0] = max_scan_corner; cm->cap_last[1] = max_scan_surf;
        cm->cap_pool = cms->cap_pool; cm->cap_work = cap_from_map;
        for (int w = 0; w < 2; ++w) for (int b = 0; b < 2; ++b) cm->pool[w][b] = cms->pool_mem[w][b] + (size_t)q * cms->cap_pool;
        if (ll_map_create(ctx, cap_from_map, cap_from_map, max_scan_corner, max_scan_surf, &cm->map) != LL_OK) { cms->err = ctx->err; ok = false; }
    }
    if (!ok) { ctx->err = cms->err; ll_cubemaps_destroy(cms); return LL_ERR_HIP; }
    *out = cms;
    return LL_OK;
}

/* the copies that gather those cubes of map cm into the search clouds of sequence q's own ll_map (:1803-1808); n_from[w]: their sizes */
static int cms_gather(ll_cubemaps *cms, int q, const ll_cubemap *cm, const int *valid, int n_valid, std::vector<CmsCopy> &ops, int n_from[2])
{
    ll_map *m = cms->cm[q]->map;
    for (int w = 0; w < 2; ++w) {
        size_t tot = 0;
        for (int v = 0; v < n_valid; ++v) {
            const int c = valid[v];
            if (cm->cnt[w][c] > 0) { ops.push_back({cm->pool[w][cm->cur[w]] + cm->off[w][c], nullptr, m->d_map[w] + tot, cm->cnt[w][c], 0}); tot += (size_t)cm->cnt[w][c]; }
        }
        if (tot > (size_t)m->cap_map[w]) { cms->err = "sequence " + std::to_string(q) + ": the valid cubes hold more points than the search cloud capacity"; return LL_ERR_CAPACITY; }
        n_from[w] = (int)tot;
    }
    return LL_OK;
}

static int cms_check_scans(ll_cubemaps *cms, const std::vector<int> &run, const std::vector<int> n_in[2])
{
    for (int r = 0; r < (int)run.size(); ++r)
        if (n_in[0][r] > cms->cap_last[0] || n_in[1][r] > cms->cap_last[1]) {
            cms->err = "sequence " + std::to_string(run[r]) + ": scan cloud larger than the capacity given to ll_cubemaps_create"; return LL_ERR_CAPACITY;
        }
    return LL_OK;
}

/* the rest of prepare once `ops` holds every running sequence's gather (n_from[w][r] points): the scans (src[w][r], device,
 * n_in[w][r] points; nullptr with flat_slot[r] >= 0: the less-flat cloud of that extracted slot is flattened into place) join the
 * one copy launch, the boxes, the :1813-1821 filters, ONE synchronisation, then the grids and the stacks of every ll_map */
static int cms_prepare_finish(ll_cubemaps *cms, const std::vector<int> &run, const std::vector<const float4 *> src[2], const std::vector<int> n_in[2],
                              const std::vector<int> &flat_slot, std::vector<CmsCopy> &ops, const std::vector<int> n_from[2])
{
    ll_ctx *ctx = cms->ctx;
    hipStream_t st = ctx->stream;
    const int R = (int)run.size();
    std::vector<int> seg_off[2];
    for (int w = 0; w < 2; ++w) {                                                  /* the scans back to back, one segment each */
        seg_off[w].assign(R + 1, 0);
        for (int r = 0; r < R; ++r) {
            float4 *dst = cms->d_last[w] + seg_off[w][r];
            if (n_in[w][r] > 0) {
                if (src[w][r]) ops.push_back({src[w][r], nullptr, dst, n_in[w][r], 0});
                else ll_launch_lflat_flatten(ctx->V, flat_slot[r], dst, st);
            }
            seg_off[w][r + 1] = seg_off[w][r] + n_in[w][r];
        }
    }
    int rc = cms_copy(cms, ops); if (rc) return rc;
    std::vector<CmsBox> boxes;
    for (int r = 0; r < R; ++r)
        for (int w = 0; w < 2; ++w) boxes.push_back({cms->cm[run[r]]->map->d_map[w], cms->d_bbox + 12 * r + 6 * w, n_from[w][r], 0});
    const CmsBox *d_boxes = (const CmsBox *)cms_stage(cms, boxes.data(), boxes.size() * sizeof(CmsBox));
    if (!d_boxes) return LL_ERR_HIP;
    hipLaunchKernelGGL(k_cms_bbox, dim3(2 * R), dim3(256), 0, st, d_boxes);
    for (int w = 0; w < 2; ++w)                                                    /* laserCloudCornerStack / SurfStack (:1813-1821) */
        if (seg_off[w][R] > 0) { rc = cms_voxel(cms, w, cms->d_last[w], seg_off[w], cms->d_stk_out[w], cms->d_nout + w); if (rc) return rc; }
    /* ONE synchronisation: every box and every stack size */
    std::vector<int> bbox((size_t)R * 12), n_stk[2] = {std::vector<int>(R, 0), std::vector<int>(R, 0)};
    {
        int *pin = (int *)ll_pinned_scratch((size_t)R * 14 * sizeof(int));
        if (!pin) { cms->err = "no page-locked scratch"; return LL_ERR_HIP; }
        CMS_HIP(hipMemcpyAsync(pin, cms->d_bbox, (size_t)R * 12 * sizeof(int), hipMemcpyDeviceToHost, st));
        for (int w = 0; w < 2; ++w)
            if (seg_off[w][R] > 0) CMS_HIP(hipMemcpyAsync(pin + (size_t)R * (12 + w), cms->W[w].seg_count, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, st));
        rc = cms_sync(cms); if (rc) return rc;
        std::memcpy(bbox.data(), pin, (size_t)R * 12 * sizeof(int));
        for (int w = 0; w < 2; ++w)
            if (seg_off[w][R] > 0) for (int r = 0; r < R; ++r) n_stk[w][r] = n_in[w][r] > 0 ? pin[(size_t)R * (12 + w) + r] : 0;
    }
    ops.clear();
    for (int r = 0; r < R; ++r) {
        ll_map *m = cms->cm[run[r]]->map;
        for (int w = 0; w < 2; ++w) { m->M.n_map[w] = n_from[w][r]; m->M.n_stk[w] = n_stk[w][r]; }
        cms->cm[run[r]]->has_frame = true;
        ll_map_rebuild_finish(m, bbox.data() + 12 * r);                            /* kdtree setInputCloud (:1826-1827) */
    }
    for (int w = 0; w < 2; ++w) {
        int at = 0;
        for (int r = 0; r < R; ++r) {
            if (n_stk[w][r] > 0) ops.push_back({cms->d_stk_out[w] + at, nullptr, cms->cm[run[r]]->map->d_stk[w], n_stk[w][r], 0});
            at += n_stk[w][r];
        }
    }
    rc = cms_copy(cms, ops); if (rc) return rc;
    CMS_HIP(hipGetLastError());
    return LL_OK;
}

/* optimize (:1822-2100) for the prepared sequences: the :1822 gate, 2 x {knn, compact, LM}, all poses back in ONE synchronisation.
 * fit != nullptr: the residual blocks once more at the final poses and k_cms_fit (ll_localize.hip); the records come back in the
 * poses' copy -- rows of the running sequences, zeros where the gate was shut.  info != nullptr: the same pass, k_cms_fit (whose
 * squares the record needs) and k_cms_info behind it; the records ride in the same copy */
static int cms_optimize(ll_cubemaps *cms, const std::vector<int> &run, double *pose_w7, int *ran, ll_localize_fit *fit, bool may_vote,
                        ll_pose_info *info = nullptr)
{
    hipStream_t st = cms->ctx->stream;
    const int R = (int)run.size();
    int rc;
    if (!cms_stage(cms, pose_w7, (size_t)cms->S * 7 * sizeof(double), cms->d_pose)) return LL_ERR_HIP;
    std::vector<int> opt_r;
    for (int r = 0; r < R; ++r) {
        const LLMapView &M = cms->cm[run[r]]->map->M;
        if (M.n_map[0] > 10 && M.n_map[1] > 50) opt_r.push_back(r);               /* :1822 */
    }
    const int O = (int)opt_r.size();
    if (fit) for (int r = 0; r < R; ++r) std::memset(fit + run[r], 0, sizeof(ll_localize_fit));
    if (info) for (int r = 0; r < R; ++r) std::memset(info + run[r], 0, sizeof(ll_pose_info));
    if (O > 0) {
        std::vector<LLMapView> views;
        std::vector<int4> blk;
        int n_vote = 0, max_vote_stk = 0;                                           /* the sequences that vote their plane blocks */
        for (int k = 0; k < O; ++k) {
            LLMapView V = cms->cm[run[opt_r[k]]]->map->M;
            V.pose = cms->d_pose + 7 * run[opt_r[k]];
            if (!may_vote) V.ctr = nullptr;                                         /* a read-only frame never votes (ll_map_vote.hip) */
            if (V.ctr) { ++n_vote; max_vote_stk = std::max(max_vote_stk, V.n_stk[1]); }
            views.push_back(V);
            for (int w = 0; w < 2; ++w) for (int f = 0; f < V.n_stk[w]; f += LL_KNNB) blk.push_back(make_int4(k, w, f, 0));
        }
        const LLMapView *d_views = (const LLMapView *)cms_stage(cms, views.data(), views.size() * sizeof(LLMapView));
        const int4 *d_blk = blk.empty() ? nullptr : (const int4 *)cms_stage(cms, blk.data(), blk.size() * sizeof(int4));
        if (!d_views || (!blk.empty() && !d_blk)) return LL_ERR_HIP;
        const LLLmOpt o = ll_to_dev_opt(nullptr);
        for (int it = 0; it < 2; ++it) {                                           /* :1832 */
            if (!blk.empty()) hipLaunchKernelGGL(k_cms_knn, dim3((unsigned)blk.size()), dim3(LL_KNNB), 0, st, d_views, d_blk);
            hipLaunchKernelGGL(k_cms_compact, dim3(2 * O), dim3(256), 0, st, d_views);
            if (n_vote > 0) ll_map_launch_vote(d_views, O, max_vote_stk, st);      /* the views without ctr return at once */
            hipLaunchKernelGGL(k_cms_lm, dim3(O), dim3(256), 0, st, d_views, o);
        }
        if (fit || info) {                                                         /* the blocks at the final pose, reduced */
            if (!blk.empty()) hipLaunchKernelGGL(k_cms_knn, dim3((unsigned)blk.size()), dim3(LL_KNNB), 0, st, d_views, d_blk);
            hipLaunchKernelGGL(k_cms_compact, dim3(2 * O), dim3(256), 0, st, d_views);
            ll_launch_cms_fit(d_views, O, cms->d_pose, cms->d_fit, st);
            if (info) ll_launch_cms_info(d_views, O, cms->d_pose, cms->d_fit, cms->d_info, st);
        }
        CMS_HIP(hipGetLastError());
        const size_t pose_bytes = (size_t)cms->S * 7 * sizeof(double), fit_bytes = (size_t)cms->S * sizeof(ll_localize_fit);
        const size_t bytes = pose_bytes + (fit || info ? fit_bytes : 0) + (info ? (size_t)cms->S * sizeof(ll_pose_info) : 0);
        double *pin = (double *)ll_pinned_scratch(bytes);
        if (!pin) { cms->err = "no page-locked scratch"; return LL_ERR_HIP; }
        CMS_HIP(hipMemcpyAsync(pin, cms->d_pose, bytes, hipMemcpyDeviceToHost, st));
        rc = cms_sync(cms); if (rc) return rc;
        for (int k = 0; k < O; ++k) std::memcpy(pose_w7 + 7 * run[opt_r[k]], pin + 7 * run[opt_r[k]], 7 * sizeof(double));
        if (fit) for (int k = 0; k < O; ++k) std::memcpy(fit + run[opt_r[k]], (const unsigned char *)pin + pose_bytes + (size_t)run[opt_r[k]] * sizeof(ll_localize_fit), sizeof(ll_localize_fit));
        if (info) for (int k = 0; k < O; ++k) std::memcpy(info + run[opt_r[k]], (const unsigned char *)pin + pose_bytes + fit_bytes + (size_t)run[opt_r[k]] * sizeof(ll_pose_info), sizeof(ll_pose_info));
    }
    int bad = -1;
    for (int r = 0, k = 0; r < R; ++r) {
        const bool opt = k < O && opt_r[k] == r;
        bool nan = false;
        if (opt) { ++k; for (int j = 0; j < 7; ++j) nan = nan || std::isnan(pose_w7[7 * run[r] + j]); }
        if (ran) ran[run[r]] = opt && !nan;
        if (nan && bad < 0) bad = run[r];
    }
    if (bad >= 0) {
        cms->err = "sequence " + std::to_string(bad) + ": the mapping solve returned an undefined pose (the input pose was NaN): set a pose and solve again";
        return LL_ERR_STATE;
    }
    return LL_OK;
}

/* one frame for the running sequences run[r]: their scans are src[w][r] (device, n_in[w][r] points; nullptr with flat_slot[r] >= 0:
 * the less-flat cloud of that extracted slot is flattened into place) */
static int cms_frame(ll_cubemaps *cms, const std::vector<int> &run, const std::vector<const float4 *> src[2], const std::vector<int> n_in[2],
                     const std::vector<int> &flat_slot, double *pose_w7, int *ran)
{
    ll_ctx *ctx = cms->ctx;
    hipStream_t st = ctx->stream;
    const int R = (int)run.size();
    int rc = cms_check_scans(cms, run, n_in); if (rc) return rc;
    /* ---------------- prepare (:1584-1821) */
    std::vector<CmsCopy> ops;
    std::vector<int> n_from[2] = {std::vector<int>(R), std::vector<int>(R)};
    for (int r = 0; r < R; ++r) {
        ll_cubemap *cm = cms->cm[run[r]];
        int nf[2];
        cm_follow(*cm, pose_w7 + 7 * run[r] + 4);                                  /* centre cube, shift loops, valid cubes (:1584-1801) */
        rc = cms_gather(cms, run[r], cm, cm->valid, cm->n_valid, ops, nf); if (rc) return rc;
        n_from[0][r] = nf[0]; n_from[1][r] = nf[1];
    }
    rc = cms_prepare_finish(cms, run, src, n_in, flat_slot, ops, n_from); if (rc) return rc;

    /* ---------------- optimize (:1822-2100) */
    rc = cms_optimize(cms, run, pose_w7, ran, nullptr, true); if (rc) return rc;

    /* ---------------- update (:2103-2165) */
    CMS_HIP(hipMemsetAsync(cms->d_addcnt, 0, (size_t)R * 2 * (CM_N + 1) * sizeof(int), st));
    std::vector<CmsAssign> recs;
    std::vector<int2> ablk;
    std::vector<int> toff[2] = {std::vector<int>(R + 1, 0), std::vector<int>(R + 1, 0)};
    for (int w = 0; w < 2; ++w)
        for (int r = 0; r < R; ++r) {
            ll_cubemap *cm = cms->cm[run[r]];
            const int ns = cm->map->M.n_stk[w], at = toff[w][r];
            toff[w][r + 1] = at + ns;
            if (ns <= 0) continue;
            CmsAssign A;
            A.stk = cm->map->d_stk[w]; A.pose = cms->d_pose + 7 * run[r];
            A.tp = cms->d_tp[w] + at; A.keys = cms->d_keys[w] + at; A.vals = cms->d_vals[w] + at;
            A.addcnt = cms->d_addcnt + ((size_t)r * 2 + w) * (CM_N + 1);
            A.n = ns; for (int k = 0; k < 3; ++k) A.cen[k] = cm->cen[k];
            for (int f = 0; f < ns; f += 256) ablk.push_back(make_int2((int)recs.size(), f));
            recs.push_back(A);
        }
    if (!recs.empty()) {
        const CmsAssign *d_recs = (const CmsAssign *)cms_stage(cms, recs.data(), recs.size() * sizeof(CmsAssign));
        const int2 *d_ablk = (const int2 *)cms_stage(cms, ablk.data(), ablk.size() * sizeof(int2));
        if (!d_recs || !d_ablk) return LL_ERR_HIP;
        hipLaunchKernelGGL(k_cms_assign, dim3((unsigned)ablk.size()), dim3(256), 0, st, d_recs, d_ablk);
        for (const CmsAssign &A : recs) {                                          /* by cube, stack order kept */
            if (ll_sort_pairs_reads_back(A.n)) ++cms->syncs;
            if (ll_sort_pairs(A.keys, A.vals, cms->WS.keys, cms->WS.vals, A.n, cms->WS.hist, cms->WS.tile_sum, cms->WS.or_and, st)) { cms->err = "sort by cube: read-back failed"; return LL_ERR_HIP; }
        }
    }
    std::vector<int> addcnt_all((size_t)R * 2 * (CM_N + 1));
    {
        int *pin = (int *)ll_pinned_scratch(addcnt_all.size() * sizeof(int));
        if (!pin) { cms->err = "no page-locked scratch"; return LL_ERR_HIP; }
        CMS_HIP(hipMemcpyAsync(pin, cms->d_addcnt, addcnt_all.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        rc = cms_sync(cms); if (rc) return rc;
        std::memcpy(addcnt_all.data(), pin, addcnt_all.size() * sizeof(int));
    }
    /* one voxel-grid segment per valid cube of every sequence: its cloud, then its new points (:2119-2125, :2151-2165) */
    std::vector<CmPlan> plan(2 * R);
    std::vector<int> useg[2], seg0[2] = {std::vector<int>(R, 0), std::vector<int>(R, 0)};
    ops.clear();
    auto new_points = [&](int r, int w) { return addcnt_all.data() + ((size_t)r * 2 + w) * (CM_N + 1); };
    /* the pieces of a plan or a commit of sequence r, type w as copies: a cube's cloud out of `from`, then its new points in by-cube order */
    auto copies = [&](const std::vector<CmPiece> &pieces, int r, int w, const float4 *from, float4 *to) {
        for (const CmPiece &e : pieces) {
            if (e.old_cnt > 0) ops.push_back({from + e.old_off, nullptr, to + e.dst, e.old_cnt, 0});
            if (e.new_cnt > 0) ops.push_back({cms->d_tp[w] + toff[w][r], cms->d_vals[w] + toff[w][r] + e.new_first, to + e.dst + e.old_cnt, e.new_cnt, 0});
        }
    };
    for (int w = 0; w < 2; ++w) {
        useg[w].assign(1, 0);
        for (int r = 0; r < R; ++r) {
            const ll_cubemap *cm = cms->cm[run[r]];
            const CmPlan &P = plan[2 * r + w] = cm_plan(*cm, w, cm->valid, cm->n_valid, new_points(r, w));
            if (P.seg_off.back() > cms->cap_work) { cms->err = "sequence " + std::to_string(run[r]) + ": the valid cubes hold more points than the filter workspace"; return LL_ERR_CAPACITY; }
            const int start = useg[w].back();
            seg0[w][r] = (int)useg[w].size() - 1;
            copies(P.pieces, r, w, cm->pool[w][cm->cur[w]], cms->d_work[w] + start);
            for (int v = 1; v <= cm->n_valid; ++v) useg[w].push_back(start + P.seg_off[v]);
        }
    }
    rc = cms_copy(cms, ops); if (rc) return rc;
    for (int w = 0; w < 2; ++w)
        if (useg[w].back() > 0) { rc = cms_voxel(cms, w, cms->d_work[w], useg[w], cms->d_out[w], cms->d_nout + 2 + w); if (rc) return rc; }
    std::vector<int> seg_count[2];
    {
        const size_t n0 = useg[0].size() - 1, n1 = useg[1].size() - 1;
        int *pin = (int *)ll_pinned_scratch((n0 + n1 + 2) * sizeof(int));
        if (!pin) { cms->err = "no page-locked scratch"; return LL_ERR_HIP; }
        if (useg[0].back() > 0 && n0) CMS_HIP(hipMemcpyAsync(pin, cms->W[0].seg_count, n0 * sizeof(int), hipMemcpyDeviceToHost, st));
        if (useg[1].back() > 0 && n1) CMS_HIP(hipMemcpyAsync(pin + n0, cms->W[1].seg_count, n1 * sizeof(int), hipMemcpyDeviceToHost, st));
        rc = cms_sync(cms); if (rc) return rc;
        seg_count[0].assign(n0, 0); seg_count[1].assign(n1, 0);
        if (useg[0].back() > 0) std::memcpy(seg_count[0].data(), pin, n0 * sizeof(int));
        if (useg[1].back() > 0) std::memcpy(seg_count[1].data(), pin + n0, n1 * sizeof(int));
    }
    /* Will it fit?  Decided for every sequence and both cloud types before any pair table changes */
    std::vector<size_t> need((size_t)R * 2);
    for (int w = 0; w < 2; ++w)
        for (int r = 0; r < R; ++r) {
            const ll_cubemap *cm = cms->cm[run[r]];
            std::string why;
            if (!cm_fit(*cm, w, plan[2 * r + w], cm->valid, cm->n_valid, new_points(r, w), seg_count[w].data() + seg0[w][r], &need[(size_t)2 * r + w], &why)) { cms->err = "sequence " + std::to_string(run[r]) + ": " + why; return LL_ERR_CAPACITY; }
        }
    /* ---- commit: from here on a failure leaves the pair tables half-updated (the sequences are marked unusable) ---- */
    for (int r = 0; r < R; ++r) cms->cm[run[r]]->broken = true;
    ops.clear();
    size_t out_at[2] = {0, 0};                                                     /* the filter output of a type: the sequences back to back */
    for (int r = 0; r < R; ++r) {
        ll_cubemap *cm = cms->cm[run[r]];
        for (int w = 0; w < 2; ++w) {
            const int *sc = seg_count[w].data() + seg0[w][r];
            const CmCommit K = cm_commit(*cm, w, plan[2 * r + w], cm->valid, cm->n_valid, new_points(r, w), sc, need[(size_t)2 * r + w]);
            const size_t n = std::accumulate(sc, sc + cm->n_valid, (size_t)0);
            cm_run_moves(cm, w, K.moves);                                          /* a compaction: launched at once, the copies below follow it */
            float4 *pool = cm->pool[w][cm->cur[w]];
            if (n > 0) ops.push_back({cms->d_out[w] + out_at[w], nullptr, pool + K.at, (int)n, 0});
            out_at[w] += n;
            copies(K.grow, r, w, pool, pool);
        }
    }
    rc = cms_copy(cms, ops); if (rc) return rc;                                   /* after every compaction above: stream order */
    CMS_HIP(hipGetLastError());
    for (int r = 0; r < R; ++r) cms->cm[run[r]]->broken = false;
    ++cms->frames;
    return LL_OK;
}

static int cms_check_common(ll_cubemaps *cms, const std::vector<int> &run)
{
    for (int q : run)
        if (cms->cm[q]->broken) { cms->err = "sequence " + std::to_string(q) + ": unusable, an earlier update failed half-way"; return LL_ERR_STATE; }
    return LL_OK;
}

/* ---- the slot intake of ll_cubemaps_process_slots, ll_cubemaps_localize_slots_info and cms_slots_dev.  The read-back of the scan
 * headers between the two halves stays with the caller: cms_slots_dev folds the poses and `extra` into the same synchronisation */
/* run: the sequences whose slot is not -1.  check_range (the public entry points): a slot outside the batch and a slot used by
 * two sequences are refused, in that order; without it (ll_drives.hip hands out the slots itself) any negative slot sits out */
static int cms_running_slots(ll_cubemaps *cms, const int *slots, bool check_range, std::vector<int> &run)
{
    const int batch = cms->ctx->p.batch;
    std::vector<char> used(check_range ? batch : 0, 0);
    for (int q = 0; q < cms->S; ++q) {
        const int s = slots[q];
        if (check_range ? s == -1 : s < 0) continue;
        if (check_range) {
            if (s < -1 || s >= batch) { cms->err = "sequence " + std::to_string(q) + ": slot out of range"; return LL_ERR_ARG; }
            if (used[s]) { cms->err = "sequence " + std::to_string(q) + ": slot " + std::to_string(s) + " is used by two sequences"; return LL_ERR_ARG; }
            used[s] = 1;
        }
        run.push_back(q);
    }
    return LL_OK;
}

/* the headers h[r] of the slots of the running sequences -> their scan clouds: src[w][r], n_in[w][r], and flat[r] = the slot whose
 * ring-strided less-flat cloud is flattened into place (-1: none).  A status other than 0 is refused; allow_empty (the drives):
 * LL_ERR_EMPTY runs with empty clouds, and the refusal names the status */
static int cms_slot_scans(ll_cubemaps *cms, const int *slots, const std::vector<int> &run, const std::vector<ScanHdr> &h, bool allow_empty,
                          std::vector<const float4 *> src[2], std::vector<int> n_in[2], std::vector<int> &flat)
{
    const int R = (int)run.size();
    const LLView &V = cms->ctx->V;
    for (int w = 0; w < 2; ++w) { src[w].assign(R, nullptr); n_in[w].assign(R, 0); }
    flat.assign(R, -1);
    for (int r = 0; r < R; ++r) {
        const int s = slots[run[r]];
        const bool empty = allow_empty && h[r].status == LL_ERR_EMPTY;
        if (h[r].status != 0 && !empty) {
            const std::string why = allow_empty ? "the scan registration refused the slot's scan (status " + std::to_string(h[r].status) + ")" : "the slot holds no extracted scan";
            cms->err = "sequence " + std::to_string(run[r]) + ": " + why;
            return LL_ERR_STATE;
        }
        src[0][r] = V.lsharp + (size_t)s * V.cap_lsharp; n_in[0][r] = empty ? 0 : h[r].n_less_sharp;
        n_in[1][r] = empty ? 0 : h[r].n_less_flat;
        if (h[r].lf_strided) { src[1][r] = nullptr; flat[r] = s; } else src[1][r] = V.lflat + (size_t)s * V.LFS;
    }
    return LL_OK;
}

extern "C" int ll_cubemaps_process_slots(ll_cubemaps *cms, const int *slots, double *pose_w7, int *ran)
{
    if (!cms || !slots || !pose_w7) return LL_ERR_ARG;
    ll_ctx *ctx = cms->ctx;
    std::vector<int> run;
    int rc = cms_running_slots(cms, slots, true, run); if (rc) return rc;
    rc = cms_check_common(cms, run); if (rc) return rc;
    if (run.empty()) return LL_OK;
    CMS_HIP(hipSetDevice(ctx->device));
    cms->par ^= 1; cms->ar[cms->par].used = 0;
    const int R = (int)run.size();
    std::vector<ScanHdr> h(R);
    {
        ScanHdr *pin = (ScanHdr *)ll_pinned_scratch((size_t)R * sizeof(ScanHdr));
        if (!pin) { cms->err = "no page-locked scratch"; return LL_ERR_HIP; }
        for (int r = 0; r < R; ++r) CMS_HIP(hipMemcpyAsync(pin + r, ctx->V.hdr + slots[run[r]], sizeof(ScanHdr), hipMemcpyDeviceToHost, ctx->stream));
        rc = cms_sync(cms); if (rc) return rc;
        std::memcpy(h.data(), pin, (size_t)R * sizeof(ScanHdr));
    }
    std::vector<const float4 *> src[2];
    std::vector<int> n_in[2], flat;
    rc = cms_slot_scans(cms, slots, run, h, false, src, n_in, flat); if (rc) return rc;
    return cms_frame(cms, run, src, n_in, flat, pose_w7, ran);
}

extern "C" int ll_cubemaps_process(ll_cubemaps *cms, const ll_point *const *corner_last, const int *n_corner, const ll_point *const *surf_last,
                                   const int *n_surf, double *pose_w7, int *ran)
{
    if (!cms || !corner_last || !n_corner || !surf_last || !n_surf || !pose_w7) return LL_ERR_ARG;
    std::vector<int> run;
    for (int q = 0; q < cms->S; ++q) {
        if (n_corner[q] < 0 || n_surf[q] < 0 || (!corner_last[q] && n_corner[q] > 0) || (!surf_last[q] && n_surf[q] > 0)) {
            cms->err = "sequence " + std::to_string(q) + ": bad scan clouds"; return LL_ERR_ARG;
        }
        if (corner_last[q] || surf_last[q]) run.push_back(q);
    }
    int rc = cms_check_common(cms, run); if (rc) return rc;
    if (run.empty()) return LL_OK;
    CMS_HIP(hipSetDevice(cms->ctx->device));
    cms->par ^= 1; cms->ar[cms->par].used = 0;
    const int R = (int)run.size();
    std::vector<const float4 *> src[2] = {std::vector<const float4 *>(R), std::vector<const float4 *>(R)};
    std::vector<int> n_in[2] = {std::vector<int>(R), std::vector<int>(R)}, flat(R, -1);
    for (int r = 0; r < R; ++r) {
        const int q = run[r];
        n_in[0][r] = n_corner[q]; n_in[1][r] = n_surf[q];
        for (int w = 0; w < 2; ++w) {
            if (n_in[w][r] > cms->cap_last[w]) { cms->err = "sequence " + std::to_string(q) + ": scan cloud larger than the capacity given to ll_cubemaps_create"; return LL_ERR_CAPACITY; }
            const ll_point *p = w ? surf_last[q] : corner_last[q];
            src[w][r] = n_in[w][r] > 0 ? (const float4 *)cms_stage(cms, p, (size_t)n_in[w][r] * sizeof(ll_point)) : nullptr;
            if (n_in[w][r] > 0 && !src[w][r]) return LL_ERR_HIP;
        }
    }
    return cms_frame(cms, run, src, n_in, flat, pose_w7, ran);
}

/* one READ-ONLY frame: sequence run[r] localises against map map_of[run[r]].  No shift loops: the centre cube in the indices the
 * map has, the cubes around it that lie inside the array (cm_valid_cubes skips the others: they hold nothing), the shared
 * prepare and optimize, no update.  Nothing of any ll_cubemap is written: the valid list is a local, the workspace is the
 * reader's ll_map.  Every refusal comes before the first launch. */
static int cms_localize(ll_cubemaps *cms, const std::vector<int> &run, const int *map_of, const std::vector<const float4 *> src[2],
                        const std::vector<int> n_in[2], const std::vector<int> &flat_slot, double *pose_w7, int *ran, ll_localize_fit *fit,
                        ll_pose_info *info)
{
    const int R = (int)run.size();
    int rc = cms_check_scans(cms, run, n_in); if (rc) return rc;
    std::vector<CmsCopy> ops;
    std::vector<int> n_from[2] = {std::vector<int>(R), std::vector<int>(R)};
    for (int r = 0; r < R; ++r) {
        const ll_cubemap *cm = cms->cm[map_of ? map_of[run[r]] : run[r]];
        int cc[3], nf[2], valid[125];
        cm_centre(*cm, pose_w7 + 7 * run[r] + 4, cc);
        const int n_valid = cm_valid_cubes(cc, valid);
        rc = cms_gather(cms, run[r], cm, valid, n_valid, ops, nf); if (rc) return rc;
        n_from[0][r] = nf[0]; n_from[1][r] = nf[1];
    }
    rc = cms_prepare_finish(cms, run, src, n_in, flat_slot, ops, n_from); if (rc) return rc;
    return cms_optimize(cms, run, pose_w7, ran, fit, false, info);
}

/* the maps the running sequences read: inside 0..S-1 and usable */
static int cms_check_read_maps(ll_cubemaps *cms, const std::vector<int> &run, const int *map_of)
{
    for (int q : run) {
        const int m = map_of ? map_of[q] : q;
        if (m < 0 || m >= cms->S) { cms->err = "sequence " + std::to_string(q) + ": map_of = " + std::to_string(m) + " is no map"; return LL_ERR_ARG; }
    }
    for (int q : run) {
        const int m = map_of ? map_of[q] : q;
        if (cms->cm[m]->broken) { cms->err = "sequence " + std::to_string(q) + ": map " + std::to_string(m) + " is unusable, an earlier update failed half-way"; return LL_ERR_STATE; }
    }
    return LL_OK;
}

extern "C" int ll_cubemaps_localize_slots(ll_cubemaps *cms, const int *slots, const int *map_of, double *pose_w7, int *ran, ll_localize_fit *fit)
{
    return ll_cubemaps_localize_slots_info(cms, slots, map_of, pose_w7, ran, fit, nullptr);
}

extern "C" int ll_cubemaps_localize_slots_info(ll_cubemaps *cms, const int *slots, const int *map_of, double *pose_w7, int *ran, ll_localize_fit *fit,
                                               ll_pose_info *info)
{
    if (!cms || !slots || !pose_w7) return LL_ERR_ARG;
    if (info) std::memset(info, 0, (size_t)cms->S * sizeof(ll_pose_info));          /* also for a sequence that sits out, and when the call is refused */
    ll_ctx *ctx = cms->ctx;
    std::vector<int> run;
    int rc = cms_running_slots(cms, slots, true, run); if (rc) return rc;
    rc = cms_check_read_maps(cms, run, map_of); if (rc) return rc;
    if (run.empty()) return LL_OK;
    CMS_HIP(hipSetDevice(ctx->device));
    cms->par ^= 1; cms->ar[cms->par].used = 0;
    const int R = (int)run.size();
    std::vector<ScanHdr> h(R);
    {
        ScanHdr *pin = (ScanHdr *)ll_pinned_scratch((size_t)R * sizeof(ScanHdr));
        if (!pin) { cms->err = "no page-locked scratch"; return LL_ERR_HIP; }
        for (int r = 0; r < R; ++r) CMS_HIP(hipMemcpyAsync(pin + r, ctx->V.hdr + slots[run[r]], sizeof(ScanHdr), hipMemcpyDeviceToHost, ctx->stream));
        rc = cms_sync(cms); if (rc) return rc;
        std::memcpy(h.data(), pin, (size_t)R * sizeof(ScanHdr));
    }
    std::vector<const float4 *> src[2];
    std::vector<int> n_in[2], flat;
    rc = cms_slot_scans(cms, slots, run, h, false, src, n_in, flat); if (rc) return rc;
    return cms_localize(cms, run, map_of, src, n_in, flat, pose_w7, ran, fit, info);
}

static int cms_seq(ll_cubemaps *cms, int q)
{
    if (q < 0 || q >= cms->S) { cms->err = "sequence index out of range"; return LL_ERR_ARG; }
    return LL_OK;
}

extern "C" int ll_cubemaps_info(ll_cubemaps *cms, int q, int *cen3, int *counts4)
{
    if (!cms) return LL_ERR_ARG;
    int rc = cms_seq(cms, q); if (rc) return rc;
    return ll_cubemap_info(cms->cm[q], cen3, counts4);
}

extern "C" int ll_cubemaps_download_cloud(ll_cubemaps *cms, int q, int which, ll_point *out, int cap, int *n)
{
    if (!cms) return LL_ERR_ARG;
    int rc = cms_seq(cms, q); if (rc) return rc;
    rc = ll_cubemap_download_cloud(cms->cm[q], which, out, cap, n);
    if (rc) cms->err = cms->cm[q]->err;
    return rc;
}

extern "C" int ll_cubemaps_download_cube(ll_cubemaps *cms, int q, int surf, int cube_index, ll_point *out, int cap, int *n)
{
    if (!cms) return LL_ERR_ARG;
    int rc = cms_seq(cms, q); if (rc) return rc;
    rc = ll_cubemap_download_cube(cms->cm[q], surf, cube_index, out, cap, n);
    if (rc) cms->err = cms->cm[q]->err;
    return rc;
}

/* the mapping vote (ll_map_vote.hip) per sequence: on[q] != 0 votes sequence q's plane blocks in ll_cubemaps_process* from now on (the switch
 * of its own ll_map; it persists until changed).  ll_cubemaps_localize_slots never votes.  Refusals come before any switch changes. */
extern "C" int ll_cubemaps_set_vote(ll_cubemaps *cms, const int *on)
{
    if (!cms) return LL_ERR_ARG;
    if (!on) { cms->err = "ll_cubemaps_set_vote: on is NULL"; return LL_ERR_ARG; }
    for (int q = 0; q < cms->S; ++q)
        if (on[q] != 0 && on[q] != 1) { cms->err = "sequence " + std::to_string(q) + ": on must be 0 or 1"; return LL_ERR_ARG; }
    for (int q = 0; q < cms->S; ++q) {
        ll_map *m = cms->cm[q]->map;
        if ((m->M.ctr != nullptr) == (on[q] != 0)) continue;
        const int rc = ll_map_set_vote(m, on[q]);
        if (rc) { cms->err = "sequence " + std::to_string(q) + ": " + m->err; return rc; }
    }
    return LL_OK;
}

/* host synchronisations and frames since create (a frame = one process call that ran at least one sequence) */
extern "C" int ll_cubemaps_stats(const ll_cubemaps *cms, long long *syncs, long long *frames)
{
    if (!cms) return LL_ERR_ARG;
    if (syncs) *syncs = cms->syncs;
    if (frames) *frames = cms->frames;
    return LL_OK;
}

/* sequence q back to what ll_cubemaps_create gave it: centre, pair tables, pool cursors, gathered-cloud counts (the pools' contents
 * are dead: nothing reads a pool beyond its tables) */
extern "C" int ll_cubemaps_reset(ll_cubemaps *cms, int q)
{
    if (!cms) return LL_ERR_ARG;
    int rc = cms_seq(cms, q); if (rc) return rc;
    ll_cubemap *cm = cms->cm[q];
    cm->cen[0] = 10; cm->cen[1] = 10; cm->cen[2] = 5;
    for (int w = 0; w < 2; ++w) {
        cm->top[w] = 0; cm->cur[w] = 0;
        std::fill(cm->off[w].begin(), cm->off[w].end(), 0); std::fill(cm->cnt[w].begin(), cm->cnt[w].end(), 0);
        cm->map->M.n_map[w] = 0; cm->map->M.n_stk[w] = 0;
    }
    cm->n_valid = 0;
    cm->broken = false; cm->has_frame = false;
    return LL_OK;
}

/* ------------------------------------------------------------------ map export (:2173-2203 for any subset of the sequences)
 * Host bookkeeping: the sizes of the selected clouds.  T != nullptr: also the segment table of the gather, numbered by T */
static int cms_export_table(ll_cubemaps *cms, const int *which, long long *offset, LLTiler *T, std::vector<LLExpSeg> *segs, long long *total)
{
    for (int q = 0; q < cms->S; ++q) {
        if (which[q] < LL_MAP_NONE || which[q] > LL_MAP_ALL) { cms->err = "sequence " + std::to_string(q) + ": which must be LL_MAP_NONE, LL_MAP_SURROUND or LL_MAP_ALL"; return LL_ERR_ARG; }
        if (which[q] != LL_MAP_NONE && cms->cm[q]->broken) { cms->err = "sequence " + std::to_string(q) + ": unusable, an earlier update failed half-way"; return LL_ERR_STATE; }
    }
    long long at = 0;
    for (int q = 0; q < cms->S; ++q) {
        if (offset) offset[q] = at;
        at += llx_segments(cms->cm[q], which[q], at, T, segs);
    }
    if (offset) offset[cms->S] = at;
    *total = at;
    return LL_OK;
}

extern "C" int ll_cubemaps_export_sizes(ll_cubemaps *cms, const int *which, long long *offset)
{
    if (!cms || !which || !offset) return LL_ERR_ARG;
    long long total = 0;
    return cms_export_table(cms, which, offset, nullptr, nullptr, &total);
}

extern "C" int ll_cubemaps_export(ll_cubemaps *cms, const int *which, ll_point *out, long long cap, long long *offset)
{
    if (!cms || !which) return LL_ERR_ARG;
    if (cap < 0) { cms->err = "map export: negative capacity"; return LL_ERR_ARG; }
    const auto t0 = std::chrono::steady_clock::now();
    LLTiler T{llx_tile()};
    std::vector<LLExpSeg> segs;
    long long total = 0;
    int rc = cms_export_table(cms, which, offset, &T, &segs, &total); if (rc) return rc;
    if (total > 0 && !out) { cms->err = "map export: out is NULL"; return LL_ERR_ARG; }
    if (total > cap) { cms->err = "map export: " + std::to_string(total) + " points, room for " + std::to_string(cap); return LL_ERR_CAPACITY; }
    if (!T.fits()) { cms->err = "map export: too many tiles for one launch"; return LL_ERR_CAPACITY; }
    CMS_HIP(hipSetDevice(cms->ctx->device));
    cms->par ^= 1; cms->ar[cms->par].used = 0;                                     /* the last frame's copies may still read the other arena */
    const LLExpSeg *d_segs = nullptr;
    if (total > 0) { d_segs = (const LLExpSeg *)cms_stage(cms, segs.data(), segs.size() * sizeof(LLExpSeg)); if (!d_segs) return LL_ERR_HIP; }
    cms->X.ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    rc = llx_gather(cms->X, cms->ctx, d_segs, segs.size(), T.next, total, (size_t)cms->S * 2 * cms->cap_pool, T.per, out, cms->err);
    if (rc == LL_OK) ++cms->syncs;
    return rc;
}

/* the last ll_cubemaps_export: ms3 = table build (host clock), gather, copy to out (device events); counts3 = points, segments, tiles */
extern "C" int ll_cubemaps_export_timing(const ll_cubemaps *cms, double *ms3, long long *counts3)
{
    if (!cms) return LL_ERR_ARG;
    llx_timing(cms->X, ms3, counts3);
    return LL_OK;
}

/* ------------------------------------------------------------------ map import: what an LL_MAP_ALL export and the layout hold, put back
 * Host bookkeeping: with an LL_MAP_ALL export the complete state of map q */
extern "C" int ll_cubemaps_layout(ll_cubemaps *cms, int q, int *cen3, int *counts, int *valid, int *n_valid)
{
    if (!cms) return LL_ERR_ARG;
    int rc = cms_seq(cms, q); if (rc) return rc;
    if (cms->cm[q]->broken) { cms->err = "sequence " + std::to_string(q) + ": unusable, an earlier update failed half-way"; return LL_ERR_STATE; }
    return ll_cubemap_layout(cms->cm[q], cen3, counts, valid, n_valid);
}

extern "C" int ll_cubemaps_import(ll_cubemaps *cms, const int *sel, const ll_point *points, const long long *offset, const int *cen3,
                                  const int *counts, const int *valid, const int *n_valid)
{
    if (!cms) return LL_ERR_ARG;
    if (!sel || !offset || !cen3 || !counts || !valid || !n_valid) { cms->err = "map import: NULL argument"; return LL_ERR_ARG; }
    const int S = cms->S;
    /* every refusal before anything is enqueued or any table changes */
    long long lo = -1, hi = -1;
    for (int q = 0; q < S; ++q) {
        if (sel[q] != 0 && sel[q] != 1) { cms->err = "sequence " + std::to_string(q) + ": sel must be 0 or 1"; return LL_ERR_ARG; }
        if (offset[q] < 0 || offset[q + 1] < offset[q]) { cms->err = "sequence " + std::to_string(q) + ": offset is not ascending"; return LL_ERR_ARG; }
        if (!sel[q]) continue;
        std::string why;
        const int rc = llx_import_check(cms->cm[q], cen3 + 3 * q, counts + (size_t)q * 2 * CM_N, valid + (size_t)q * 125, n_valid[q], offset[q + 1] - offset[q], why);
        if (rc) { cms->err = "sequence " + std::to_string(q) + ": " + why; return rc; }
        if (offset[q + 1] > offset[q]) { if (lo < 0) lo = offset[q]; hi = offset[q + 1]; }
    }
    const long long n_up = lo < 0 ? 0 : hi - lo;
    if (n_up > 0 && !points) { cms->err = "map import: points is NULL"; return LL_ERR_ARG; }
    LLTiler T{llx_tile()};
    std::vector<LLImpSeg> segs;
    for (int q = 0; q < S; ++q)
        if (sel[q]) llx_import_segments(cms->cm[q], counts + (size_t)q * 2 * CM_N, offset[q] - (lo < 0 ? 0 : lo), T, &segs);
    if (!T.fits()) { cms->err = "map import: too many tiles for one launch"; return LL_ERR_CAPACITY; }
    CMS_HIP(hipSetDevice(cms->ctx->device));
    const bool direct = n_up > 0 && llx_is_device(points);
    float4 *src = direct ? (float4 *)points + lo : nullptr;
    if (n_up > 0 && !direct) {
        std::string why;
        src = llx_reserve(cms->X, (size_t)n_up, why);
        if (!src) { cms->err = "map import: " + why; return LL_ERR_HIP; }
    }
    cms->par ^= 1; cms->ar[cms->par].used = 0;
    const LLImpSeg *d_segs = nullptr;
    if (!segs.empty()) { d_segs = (const LLImpSeg *)cms_stage(cms, segs.data(), segs.size() * sizeof(LLImpSeg)); if (!d_segs) return LL_ERR_HIP; }
    /* ---- from here on a failure leaves the selected maps' pools half-written ---- */
    for (int q = 0; q < S; ++q) if (sel[q]) cms->cm[q]->broken = true;
    int rc = llx_scatter(cms->ctx, d_segs, segs.size(), T.next, src, direct ? nullptr : (const void *)(points + lo), (size_t)n_up, T.per, cms->err);
    if (rc) return rc;
    rc = cms_sync(cms); if (rc) return rc;                                         /* the ONE synchronisation: the caller's points may go away */
    for (int q = 0; q < S; ++q)
        if (sel[q]) llx_import_commit(cms->cm[q], cen3 + 3 * q, counts + (size_t)q * 2 * CM_N, valid + (size_t)q * 125, n_valid[q]);
    return LL_OK;
}

/* ------------------------------------------------------------------ for ll_drives (ll_drives.hip), not exported */
void llcms_begin(ll_cubemaps *cms) { cms->par ^= 1; cms->ar[cms->par].used = 0; }
void *llcms_stage(ll_cubemaps *cms, const void *src, size_t bytes) { return cms_stage(cms, src, bytes); }
double *llcms_dev_pose(ll_cubemaps *cms) { return cms->d_pose; }
long long llcms_syncs(const ll_cubemaps *cms) { return cms->syncs; }
const std::string &llcms_err(const ll_cubemaps *cms) { return cms->err; }
ll_cubemap *llcms_map(ll_cubemaps *cms, int q) { return cms->cm[q]; }
LLMapExport &llcms_export_state(ll_cubemaps *cms) { return cms->X; }
void *llcms_stage_to(ll_cubemaps *cms, const void *src, size_t bytes, void *dst) { return cms_stage(cms, src, bytes, dst); }
int llcms_sync(ll_cubemaps *cms) { return cms_sync(cms); }
int llcms_size(const ll_cubemaps *cms) { return cms->S; }
const float *llcms_leaf(const ll_cubemaps *cms) { return cms->leaf; }
LLMapMerge &llcms_merge_state(ll_cubemaps *cms) { return cms->G; }
LLMapAlign &llcms_align_state(ll_cubemaps *cms) { return cms->A; }
int llcms_fail(ll_cubemaps *cms, int rc, const std::string &msg) { cms->err = msg; return rc; }
void llcms_count_sync(ll_cubemaps *cms) { ++cms->syncs; }

/* ll_cubemaps_process_slots (map_of == nullptr) or ll_cubemaps_localize_slots with the guesses already in d_pose (rows of the
 * running sequences; llcms_begin called): they come to the host with the slot headers, in the same synchronisation, together
 * with extra_bytes from extra_dev into extra_host.  A slot whose extract status is LL_ERR_EMPTY runs with empty clouds.
 * hdr_out[q]: the header of slots[q] (running sequences). */
static int cms_slots_dev(ll_cubemaps *cms, const int *slots, const int *map_of, double *pose_w7, int *ran, ll_localize_fit *fit, ll_pose_info *info,
                         const void *extra_dev, void *extra_host, size_t extra_bytes, ScanHdr *hdr_out)
{
    ll_ctx *ctx = cms->ctx;
    std::vector<int> run;
    int rc = cms_running_slots(cms, slots, false, run); if (rc) return rc;
    rc = map_of ? cms_check_read_maps(cms, run, map_of) : cms_check_common(cms, run); if (rc) return rc;
    const int R = (int)run.size();
    const size_t pose_bytes = (size_t)cms->S * 7 * sizeof(double), hdr_at = (pose_bytes + extra_bytes + 15) & ~(size_t)15;
    std::vector<ScanHdr> h(R);
    {
        unsigned char *pin = (unsigned char *)ll_pinned_scratch(hdr_at + (size_t)R * sizeof(ScanHdr));
        if (!pin) { cms->err = "no page-locked scratch"; return LL_ERR_HIP; }
        CMS_HIP(hipMemcpyAsync(pin, cms->d_pose, pose_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (extra_bytes) CMS_HIP(hipMemcpyAsync(pin + pose_bytes, extra_dev, extra_bytes, hipMemcpyDeviceToHost, ctx->stream));
        for (int r = 0; r < R; ++r)
            CMS_HIP(hipMemcpyAsync(pin + hdr_at + (size_t)r * sizeof(ScanHdr), ctx->V.hdr + slots[run[r]], sizeof(ScanHdr), hipMemcpyDeviceToHost, ctx->stream));
        rc = cms_sync(cms); if (rc) return rc;
        std::memcpy(pose_w7, pin, pose_bytes);
        if (extra_bytes) std::memcpy(extra_host, pin + pose_bytes, extra_bytes);
        std::memcpy(h.data(), pin + hdr_at, (size_t)R * sizeof(ScanHdr));
    }
    if (R == 0) return LL_OK;
    for (int r = 0; r < R; ++r) hdr_out[run[r]] = h[r];
    std::vector<const float4 *> src[2];
    std::vector<int> n_in[2], flat;
    rc = cms_slot_scans(cms, slots, run, h, true, src, n_in, flat); if (rc) return rc;
    return map_of ? cms_localize(cms, run, map_of, src, n_in, flat, pose_w7, ran, fit, info) : cms_frame(cms, run, src, n_in, flat, pose_w7, ran);
}

int llcms_process_slots_dev(ll_cubemaps *cms, const int *slots, double *pose_w7, int *ran, const void *extra_dev, void *extra_host,
                            size_t extra_bytes, ScanHdr *hdr_out)
{
    return cms_slots_dev(cms, slots, nullptr, pose_w7, ran, nullptr, nullptr, extra_dev, extra_host, extra_bytes, hdr_out);
}

int llcms_localize_slots_dev(ll_cubemaps *cms, const int *slots, const int *map_of, double *pose_w7, int *ran, ll_localize_fit *fit, ll_pose_info *info,
                             const void *extra_dev, void *extra_host, size_t extra_bytes, ScanHdr *hdr_out)
{
    return cms_slots_dev(cms, slots, map_of, pose_w7, ran, fit, info, extra_dev, extra_host, extra_bytes, hdr_out);
}
