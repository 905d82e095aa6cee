/*
 * ll_map_align.hip -- one cube map registered to another on the device: op (dst, src, T0) estimates the rigid transform that takes
 * src's world frame into dst's with laserMapping's scan-to-map optimisation (laserMapping.cpp:1822-2095) over the WHOLE of both
 * maps: the stacks are src's corner and surf points in the order an LL_MAP_ALL export lists a type (cube 0 .. 4850, inside a cube
 * its own order), the search clouds are dst's in the same order, and a neighbour's index is its position there.  Nothing of any
 * map is written.  The per-frame path (ll_cubemaps.hip) cannot do this: its dense grid over a cloud's bounding box degenerates
 * over hundreds of metres, k_cms_lm is one workgroup per view, and an ll_map's buffers are sized for 125 cubes and one scan.
 *
 * Search structure, per distinct dst map and cloud type ("cloud"): the cube array is the first level -- a table occupied cube ->
 * slot; per slot a table of 40^3 + 1 ints over world-anchored cells of 1.25 m, which tile a 50 m cube exactly (the cube faces lie
 * at -25 + 50 k); the cloud's points reordered by (cube, cell) with the index in .w, as LLGrid3::pts carries it.  The 0.25 m over
 * the 1 m acceptance radius covers every rounding of a cell assignment, also the clamp of a point that sits on its cube's far face.
 * It is exact for points that lie in the cube the library's arithmetic (:2108-2125) gives them, which is what every frame, merge
 * and import of an export leaves.
 *   k_al_count    a workgroup takes one tile of one cube's cloud where it lies in the pool (a segment table and a binary search over
 *                 the segments' first tiles, as k_mm_assign): a src cube is copied into the flat stack, a dst cube counts its
 *                 points per cell;
 *   k_al_scan     per slot the exclusive scan of its table, from the cube's first place in the cell-ordered array;
 *   k_al_scatter  the points into cell order.  The order inside a cell is that of the atomics; the five nearest are a total order
 *                 on (distance, index), so no result depends on it.
 * Per outer iteration:
 *   k_al_knn      ll_map_knn_one's body for the 64 stack points of one (op, type, first) row of the block table: the 27 cells by
 *                 global cell coordinate, (cube, local cell) resolved per row of three x-cells -- a row that crosses a cube face is
 *                 two ranges -- all bounds first, all ranges advancing together (ll_map_search5's shape); a cell outside the
 *                 array or in an empty cube holds nothing, a query whose own cell does is searched all the same;
 *   k_al_cscan    per (op, type) the running sum of the knn workgroups' block counts;  k_al_place: the blocks in stack order;
 *   then 1 + max_num_iterations times
 *   k_al_eval     (op, chunk of AL_CHUNK blocks, edges first): the 28 sums of k_map_normal_eq in f64, written with plain stores;
 *   k_al_solve    one wave per op: the partials summed in chunk order, then ll_lm_begin_one / _accept_one / _propose_one on one
 *                 thread.  The order of every sum is fixed by (AL_CHUNK, chunk index): an op's pose has the same bits alone or
 *                 among others, and from call to call.
 * No kernel waits on another workgroup.  The fit record is one more knn / cscan / place at the final pose, k_al_eval's second
 * form (cost, sq_edge, sq_plane) and k_al_fitsum; the information record (ll_pose_info) is k_al_eval's first form once more on those
 * blocks and k_al_infosum (ll_pose_info.h), which reads the squares k_al_fitsum left.
 * The host synchronises ONCE per call, for the poses, the records and the block counts: the cube counts and offsets are host
 * bookkeeping, so the launches and the workspace are planned without a read-back.
 */
#include "ll_cubemaps.h"
#include "ll_tiles.h"
#include "ll_factor_math.h"
#include "ll_map_neq.h"
#include "ll_map_search.h"
#include "ll_pose_info.h"
#include <cmath>

#define AL_SIDE 40                           /* cells per cube side: 50 m / 1.25 m */
#define AL_CELLS (AL_SIDE * AL_SIDE * AL_SIDE)
#define AL_TAB (AL_CELLS + 1)                /* ints per slot: T[c] = first cell-ordered point of cell c, T[AL_CELLS] = end */
#define AL_TILE 1024                         /* points per workgroup of k_al_count / k_al_scatter: 256 lanes x 4 */
#define AL_CHUNK 1024                        /* residual blocks per workgroup of k_al_eval: 256 lanes x 4 */

/* one non-empty cube of a map in one role.  slot < 0: a src cube, copied to flat[base + i]; slot >= 0: a dst cube, its points go
 * to cell order in table `slot`, base = its first point's index in the cloud, at = where the cloud begins in the sorted array (the
 * tables hold positions in the sorted array, the points' .w indices in the cloud);
 * wc: the cube's place in the world (index minus the map's centre) */
struct AlSeg { const float4 *src; float4 *flat; int cnt, base, at, slot; unsigned tile0; int wc[3]; };
/* a dst cloud as the search sees it: c2s[cube] = slot or -1 */
struct AlGrid { const int *c2s; int cen[3]; int pad; };
/* what an op has beyond its LLMapView: the two dst clouds, its rows of the block table per type, its first chunk of k_al_eval */
struct AlOp { int grid[2], blk0[2], nblk[2], chunk0, pad; };

/* the cell of a map point inside its cube; a coordinate that is no number, or lies beyond the cube, goes to an edge cell */
__device__ __forceinline__ int al_local(float x, int wc)
{
    const double v = floor((((double)x + 25.0) - 50.0 * (double)wc) / 1.25);
    return !(v >= 0.0) ? 0 : (v >= (double)AL_SIDE ? AL_SIDE - 1 : (int)v);
}
__device__ __forceinline__ int al_cell(const float4 p, const int wc[3])
{
    return (al_local(p.z, wc[2]) * AL_SIDE + al_local(p.y, wc[1])) * AL_SIDE + al_local(p.x, wc[0]);
}

__global__ __launch_bounds__(256) void k_al_count(const AlSeg *seg, int nseg, int *T)
{
    const AlSeg s = seg[ll_tile_find(seg, nseg, blockIdx.x)];
    const int first = (int)(blockIdx.x - s.tile0) * AL_TILE, n = min(AL_TILE, s.cnt - first);
    float4 po[AL_TILE / 256];
#pragma unroll
    for (int k = 0; k < AL_TILE / 256; ++k) po[k] = s.src[first + min(k * 256 + (int)threadIdx.x, n - 1)];
    int *tab = T + (size_t)max(s.slot, 0) * AL_TAB;
#pragma unroll
    for (int k = 0; k < AL_TILE / 256; ++k) {
        const int i = k * 256 + (int)threadIdx.x;
        if (i >= n) continue;
        if (s.slot < 0) s.flat[s.base + first + i] = po[k];
        else atomicAdd(&tab[al_cell(po[k], s.wc) + 1], 1);         /* T[0] stays 0: the scan turns counts into first points */
    }
}

/* T[slot][c] <- slot_base[slot] (the cube's first place in the sorted array) + T[slot][0] + .. + T[slot][c - 1]: one workgroup per slot */
__global__ __launch_bounds__(256) void k_al_scan(int *T, const int *slot_base)
{
    __shared__ int sc[4];
    int *t = T + (size_t)blockIdx.x * AL_TAB;
    int base = slot_base[blockIdx.x];
    for (int b0 = 0; b0 < AL_TAB; b0 += 256) {
        const int b = b0 + (int)threadIdx.x;
        int total;
        const int pos = base + ll_block_exscan_n<4>(b < AL_TAB ? t[b] : 0, sc, total);
        if (b < AL_TAB) t[b] = pos;
        base += total;
    }
}

/* afterwards T[c + 1] has advanced from the first point of cell c to its end, the first point of cell c + 1 */
__global__ __launch_bounds__(256) void k_al_scatter(const AlSeg *seg, int nseg, int *T, float4 *sorted)
{
    const AlSeg s = seg[ll_tile_find(seg, nseg, blockIdx.x)];
    if (s.slot < 0) return;
    const int first = (int)(blockIdx.x - s.tile0) * AL_TILE, n = min(AL_TILE, s.cnt - first);
    float4 po[AL_TILE / 256];
#pragma unroll
    for (int k = 0; k < AL_TILE / 256; ++k) po[k] = s.src[first + min(k * 256 + (int)threadIdx.x, n - 1)];
    int *tab = T + (size_t)s.slot * AL_TAB;
    const int lo = s.at + s.base;                                 /* the cube's points lie at [lo, lo + cnt) of the sorted array */
#pragma unroll
    for (int k = 0; k < AL_TILE / 256; ++k) {
        const int i = k * 256 + (int)threadIdx.x;
        if (i >= n) continue;
        const int pos = atomicAdd(&tab[al_cell(po[k], s.wc) + 1], 1);
        if (pos >= lo && pos < lo + s.cnt) sorted[pos] = make_float4(po[k].x, po[k].y, po[k].z, __int_as_float(s.base + first + i));
    }
}

/* floor(g / 40) and the remainder in 0 .. 39 for any sign */
__device__ __forceinline__ void al_split(int g, int &cube, int &local)
{
    cube = g >= 0 ? g / AL_SIDE : -((AL_SIDE - 1 - g) / AL_SIDE);
    local = g - cube * AL_SIDE;
}

/* nine ranges advance together, two points of each per round (ll_map_search5's loop) */
__device__ __forceinline__ void al_scan9(const float4 *pts, int st[9], const int en[9], float sx, float sy, float sz,
                                         float bd[5], int bi[5], float4 bp[5], int &nb)
{
    for (;;) {
        float4 p[9][2];
        bool any = false;
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
            for (int u = 0; u < 2; ++u) if (st[r] + u < en[r]) { p[r][u] = pts[st[r] + u]; any = true; }
        if (!any) break;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (st[r] + u >= en[r]) continue;
                float diff = sx - p[r][u].x; float d = diff * diff;            /* FLANN L2_Simple: a = query, b = data */
                diff = sy - p[r][u].y; d += diff * diff;
                diff = sz - p[r][u].z; d += diff * diff;
                ll_five_insert<true>(bd, bi, bp, nb, d, __float_as_int(p[r][u].w), p[r][u]);
            }
            st[r] += 2;
        }
    }
}

/* exact K = 5 over the 27 cells of 1.25 m around the query, ascending (distance, index in the cloud), the points with them */
__device__ __forceinline__ void al_search5(const AlGrid &G, const int *T, const float4 *pts, float sx, float sy, float sz,
                                           float bd[5], int bi[5], float4 bp[5], int &nb)
{
    nb = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) { bd[k] = INFINITY; bi[k] = INT_MAX; bp[k] = make_float4(0.f, 0.f, 0.f, 0.f); }
    const double fx = floor(((double)sx + 25.0) / 1.25), fy = floor(((double)sy + 25.0) / 1.25), fz = floor(((double)sz + 25.0) / 1.25);
    if (!(fabs(fx) < 1e9 && fabs(fy) < 1e9 && fabs(fz) < 1e9)) return;          /* no number, or nowhere near any array */
    const int gx = (int)fx, gy = (int)fy, gz = (int)fz;
    int ca, la, cb, lb;
    al_split(gx - 1, ca, la); al_split(gx + 1, cb, lb);
    const int ia = ca + G.cen[0], ib = cb + G.cen[0];
    const bool in_a = ia >= 0 && ia < CM_W, in_b = cb != ca && ib >= 0 && ib < CM_W;
    /* the nine (z, y) rows: the slots of the one or two cubes a row's three x-cells lie in, all eighteen loads first */
    int sa[9], sb[9], row[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        int cj, lj, ck, lk;
        al_split(gy + (r % 3) - 1, cj, lj); al_split(gz + (r / 3) - 1, ck, lk);
        const int j = cj + G.cen[1], k = ck + G.cen[2];
        const bool in = j >= 0 && j < CM_H && k >= 0 && k < CM_D;
        const int cube = ia + CM_W * j + CM_W * CM_H * k;
        row[r] = (lk * AL_SIDE + lj) * AL_SIDE;
        sa[r] = (in && in_a) ? G.c2s[cube] : -1;
        sb[r] = (in && in_b) ? G.c2s[cube + 1] : -1;
    }
    int st[9], en[9], st2[9], en2[9];
    const int la_end = (cb != ca) ? AL_SIDE - 1 : lb;              /* the row's last cell inside the first cube */
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        st[r] = en[r] = st2[r] = en2[r] = 0;
        if (sa[r] >= 0) { const int *t = T + (size_t)sa[r] * AL_TAB + row[r]; st[r] = t[la]; en[r] = t[la_end + 1]; }
        if (sb[r] >= 0) { const int *t = T + (size_t)sb[r] * AL_TAB + row[r]; st2[r] = t[0]; en2[r] = t[lb + 1]; }
    }
    al_scan9(pts, st, en, sx, sy, sz, bd, bi, bp, nb);
    al_scan9(pts, st2, en2, sx, sy, sz, bd, bi, bp, nb);           /* nothing to do unless the rows cross a cube face in x */
}

template <bool CORNER>
__device__ __forceinline__ bool al_knn_one(const LLMapView &M, const AlGrid &G, const int *T, const float4 *pts, int i)
{
    const int which = CORNER ? 0 : 1;
    if (i >= M.n_stk[which]) return false;
    float sx, sy, sz;
    ll_map_to_world(M.pose, M.stk[which][i], sx, sy, sz);
    float bd[5]; int bi[5]; float4 bp[5]; int nb;
    al_search5(G, T, pts, sx, sy, sz, bd, bi, bp, nb);
    if (nb == 5 && bd[4] < 1.0f) {                                                                     /* :1885, :1958 */
        double P5[5][3];
#pragma unroll
        for (int j = 0; j < 5; ++j) { P5[j][0] = bp[j].x; P5[j][1] = bp[j].y; P5[j][2] = bp[j].z; }
        ll_map_fit<CORNER>(M, i, P5);
        return M.ok[which][i] != 0;
    }
    M.ok[which][i] = 0;
    return false;
}

/* row b of the block table covers the LL_KNNB stack points from blk[b].z of cloud type blk[b].y of op blk[b].x */
__global__ __launch_bounds__(LL_KNNB) void k_al_knn(const LLMapView *views, const AlOp *ops, const AlGrid *grids, const int4 *blk,
                                                    const int *T, const float4 *pts, int *blkcnt)
{
    const int4 b = blk[blockIdx.x];
    const LLMapView &M = views[b.x];
    const AlGrid &G = grids[ops[b.x].grid[b.y]];
    const bool ok = b.y == 0 ? al_knn_one<true>(M, G, T, pts, b.z + threadIdx.x) : al_knn_one<false>(M, G, T, pts, b.z + threadIdx.x);
    const unsigned long long m = __ballot(ok);
    if (threadIdx.x == 0) blkcnt[blockIdx.x] = __popcll(m);
}

/* per (op, type): blkbase[b] = the blocks of the rows before b, counts[type] = all of them */
__global__ __launch_bounds__(256) void k_al_cscan(const LLMapView *views, const AlOp *ops, const int *blkcnt, int *blkbase)
{
    __shared__ int sc[4];
    const AlOp &o = ops[blockIdx.x >> 1];
    const int which = blockIdx.x & 1, b0 = o.blk0[which], nb = o.nblk[which];
    int base = 0;
    for (int c0 = 0; c0 < nb; c0 += 256) {
        const int c = c0 + (int)threadIdx.x;
        int total;
        const int pos = base + ll_block_exscan_n<4>(c < nb ? blkcnt[b0 + c] : 0, sc, total);
        if (c < nb) blkbase[b0 + c] = pos;
        base += total;
    }
    if (threadIdx.x == 0) views[blockIdx.x >> 1].counts[which] = base;
}

/* k_cms_compact's result over the block table: residual blocks in stack order */
__global__ __launch_bounds__(LL_KNNB) void k_al_place(const LLMapView *views, const int4 *blk, const int *blkbase)
{
    const int4 b = blk[blockIdx.x];
    const LLMapView &M = views[b.x];
    const int which = b.y, i = b.z + (int)threadIdx.x;
    const bool ok = i < M.n_stk[which] && M.ok[which][i];
    const unsigned long long m = __ballot(ok);
    if (!ok) return;
    const int pos = blkbase[blockIdx.x] + __popcll(m & ((1ull << threadIdx.x) - 1ull));
    ll_map_place(M, which, pos, i);
}

/* workgroup b: chunk chunks[b].y of op chunks[b].x -- blocks j0 .. j0 + AL_CHUNK - 1 of the op's edges-then-planes order, block
 * j0 + 256 k + tid on thread tid.  FIT = false: k_map_normal_eq's 28 sums; FIT = true: cost, sq_edge, sq_plane in the first
 * three.  Summed per thread, over the wave, over the four waves in wave order; part[b][28] by plain stores.  A chunk beyond the
 * op's blocks writes nothing and is never read. */
template <bool FIT>
__global__ __launch_bounds__(256) void k_al_eval(const LLMapView *views, const int2 *chunks, double *part)
{
    const int2 c = chunks[blockIdx.x];
    const LLMapView &M = views[c.x];
    const int tid = threadIdx.x;
    const int n_e = M.counts[0], n_p = M.counts[1], j0 = c.y * AL_CHUNK;
    if (j0 >= n_e + n_p) return;
    const Pose P = ll_pose_load(M.pose);
    double acc[LL_NACC];
#pragma unroll
    for (int k = 0; k < LL_NACC; ++k) acc[k] = 0.0;
    for (int u = 0; u < AL_CHUNK / 256; ++u) {
        const int j = j0 + u * 256 + tid;
        if (j < n_e) { if (FIT) ll_map_fit_edge(M, P, j, acc); else ll_map_acc_edge(M, P, j, acc); }
        else if (j < n_e + n_p) { if (FIT) ll_map_fit_plane(M, P, j - n_e, acc); else ll_map_acc_plane(M, P, j - n_e, acc); }
    }
    __shared__ double red[4][LL_NACC];
    ll_wg_sum<(FIT ? LL_FIT_NACC : LL_NACC)>(acc, red);
    if (tid < (FIT ? LL_FIT_NACC : LL_NACC)) part[(size_t)blockIdx.x * LL_NACC + tid] = ll_wg_total(red, tid);
}

/* one wave per op: round `round` of k_cms_lm's loop on the partials of the evaluation at the op's pose, summed in chunk order */
__global__ __launch_bounds__(64) void k_al_solve(const LLMapView *views, const AlOp *ops, const double *part, LLLmOpt o, int round)
{
    const LLMapView &M = views[blockIdx.x];
    const int tid = threadIdx.x, n_e = M.counts[0], n_p = M.counts[1];
    const int used = (n_e + n_p + AL_CHUNK - 1) / AL_CHUNK;
    __shared__ double stot[LL_NACC], sneq[LL_NEQ_STRIDE], sL[LL_LM_STRIDE], sp[7];
    if (tid < LL_NACC) stot[tid] = ll_partials_sum(part + (size_t)ops[blockIdx.x].chunk0 * LL_NACC, used, tid);
    for (int k = tid; k < LL_LM_STRIDE; k += 64) sL[k] = round == 0 ? 0.0 : M.lm[k];
    if (tid < 7) sp[tid] = M.pose[tid];
    __syncthreads();
    if (tid == 0) {
        ll_neq_unpack(stot, 3 * n_e + n_p, sneq);
        ll_lm_round(sL, sneq, sp, o, round);
    }
    __syncthreads();
    if (tid < 7) M.pose[tid] = sp[tid];
    for (int k = tid; k < LL_LM_STRIDE; k += 64) M.lm[k] = sL[k];
}

/* one wave per op: the record from the partials of k_al_eval<true>, summed in chunk order */
__global__ __launch_bounds__(64) void k_al_fitsum(const LLMapView *views, const AlOp *ops, const double *part, ll_localize_fit *fit)
{
    const LLMapView &M = views[blockIdx.x];
    const int tid = threadIdx.x, n_e = M.counts[0], n_p = M.counts[1];
    const int used = (n_e + n_p + AL_CHUNK - 1) / AL_CHUNK;
    __shared__ double stot[LL_FIT_NACC];
    if (tid < LL_FIT_NACC) stot[tid] = ll_partials_sum(part + (size_t)ops[blockIdx.x].chunk0 * LL_NACC, used, tid);
    __syncthreads();
    if (tid == 0) {
        ll_localize_fit F;
        F.n_edge = n_e; F.n_plane = n_p; F.cost = stot[0]; F.sq_edge = stot[1]; F.sq_plane = stot[2];
        fit[blockIdx.x] = F;
    }
}

/* one wave per op: the ll_pose_info record (ll_pose_info.h) from the partials of k_al_eval<false> at the final T, summed in chunk
 * order, and the squares k_al_fitsum left in fit[] -- launched behind it */
__global__ __launch_bounds__(64) void k_al_infosum(const LLMapView *views, const AlOp *ops, const double *part, const ll_localize_fit *fit, ll_pose_info *info)
{
    const LLMapView &M = views[blockIdx.x];
    const int tid = threadIdx.x, n_e = M.counts[0], n_p = M.counts[1];
    const int used = (n_e + n_p + AL_CHUNK - 1) / AL_CHUNK;
    __shared__ double stot[LL_NACC], work[LL_NEQ_STRIDE];
    if (tid < LL_NACC) stot[tid] = ll_partials_sum(part + (size_t)ops[blockIdx.x].chunk0 * LL_NACC, used, tid);
    __syncthreads();
    if (tid == 0) ll_info_finish(stot, fit[blockIdx.x], work, info + blockIdx.x);
}

/* ------------------------------------------------------------------ host side */
void llal_free(LLMapAlign &A)
{
    if (A.d_mem) (void)hipFree(A.d_mem);
    for (hipEvent_t e : A.ev) (void)hipEventDestroy(e);
    A = LLMapAlign();
}

#define AL_HIP(call) LL_HIP_CHECK(llcms_fail, cms, "map align: ", call, #call)

/* a map in one role: which of its cubes hold points of type w, and how many in all */
struct AlCloud { int map, w; long long n, first; int slot0, nslot; };

extern "C" int ll_cubemaps_align(ll_cubemaps *cms, const ll_merge_op *ops, int n_ops, int n_outer, const ll_lm_options *opt,
                                 double *T_w7, int *ran, ll_localize_fit *fit)
{
    return ll_cubemaps_align_info(cms, ops, n_ops, n_outer, opt, T_w7, ran, fit, nullptr);
}

extern "C" int ll_cubemaps_align_info(ll_cubemaps *cms, const ll_merge_op *ops, int n_ops, int n_outer, const ll_lm_options *opt,
                                      double *T_w7, int *ran, ll_localize_fit *fit, ll_pose_info *info)
{
    if (!cms) return LL_ERR_ARG;
    if (n_ops < 0) return llcms_fail(cms, LL_ERR_ARG, "map align: n_ops < 0");
    if (n_outer < 0) return llcms_fail(cms, LL_ERR_ARG, "map align: n_outer < 0");
    if (n_ops > 0 && !ops) return llcms_fail(cms, LL_ERR_ARG, "map align: ops is NULL");
    if (n_ops > 0 && !T_w7) return llcms_fail(cms, LL_ERR_ARG, "map align: op 0: T_w7 is NULL");
    const int S = llcms_size(cms);
    /* ---- every refusal before anything is enqueued */
    for (int i = 0; i < n_ops; ++i) {
        const ll_merge_op &o = ops[i];
        const std::string who = "map align: op " + std::to_string(i) + ": ";
        if (o.dst < 0 || o.dst >= S || o.src < 0 || o.src >= S) return llcms_fail(cms, LL_ERR_ARG, who + "dst or src is no map");
        if (o.dst == o.src) return llcms_fail(cms, LL_ERR_ARG, who + "dst and src are the same map");
    }
    for (int i = 0; i < n_ops; ++i)
        for (const int q : {ops[i].dst, ops[i].src})
            if (llcms_map(cms, q)->broken) return llcms_fail(cms, LL_ERR_STATE, "map align: op " + std::to_string(i) + ": map " + std::to_string(q) + " is unusable, an earlier update failed half-way");
    for (int i = 0; i < n_ops; ++i)
        for (int k = 0; k < 7; ++k)
            if (std::isnan(ops[i].T_w7[k])) return llcms_fail(cms, LL_ERR_STATE, "map align: op " + std::to_string(i) + ": the guess is an undefined pose (NaN)");
    LLMapAlign &A = llcms_align_state(cms);
    for (int k = 0; k < 4; ++k) A.ms[k] = 0.0;
    for (int k = 0; k < 3; ++k) A.counts[k] = 0;
    for (int i = 0; i < n_ops; ++i) {
        std::memcpy(T_w7 + 7 * i, ops[i].T_w7, 7 * sizeof(double));
        if (ran) ran[i] = 0;
        if (fit) std::memset(fit + i, 0, sizeof(ll_localize_fit));
        if (info) std::memset(info + i, 0, sizeof(ll_pose_info));
    }
    /* ---- the :1822 gate on the host's own counts; the clouds of the ops that pass: dst clouds (searched), src clouds (stacks) */
    auto total = [&](int q, int w) { long long n = 0; const ll_cubemap *cm = llcms_map(cms, q); for (int c = 0; c < CM_N; ++c) n += cm->cnt[w][c]; return n; };
    std::vector<int> run;
    std::vector<AlCloud> grids, stacks;
    std::vector<int> grid_of(2 * (size_t)S, -1), stack_of(2 * (size_t)S, -1);
    for (int i = 0; i < n_ops; ++i) {
        if (!(total(ops[i].dst, 0) > 10 && total(ops[i].dst, 1) > 50)) continue;    /* :1822 */
        run.push_back(i);
        for (int w = 0; w < 2; ++w) {
            if (grid_of[2 * ops[i].dst + w] < 0) { grid_of[2 * ops[i].dst + w] = (int)grids.size(); grids.push_back({ops[i].dst, w, total(ops[i].dst, w), 0, 0, 0}); }
            if (stack_of[2 * ops[i].src + w] < 0) { stack_of[2 * ops[i].src + w] = (int)stacks.size(); stacks.push_back({ops[i].src, w, total(ops[i].src, w), 0, 0, 0}); }
        }
    }
    const int O = (int)run.size();
    if (O == 0) return LL_OK;
    /* ---- layout: slots and sorted points of the dst clouds, flat stacks of the src clouds, the per-op buffers */
    long long n_sorted = 0, n_flat = 0, n_slot = 0;
    for (AlCloud &g : grids) {
        const ll_cubemap *cm = llcms_map(cms, g.map);
        g.first = n_sorted; n_sorted += g.n; g.slot0 = (int)n_slot;
        for (int c = 0; c < CM_N; ++c) if (cm->cnt[g.w][c] > 0) ++g.nslot;
        n_slot += g.nslot;
    }
    for (AlCloud &s : stacks) { s.first = n_flat; n_flat += s.n; }
    if (n_sorted > (1ll << 30) || n_flat > (1ll << 30)) return llcms_fail(cms, LL_ERR_CAPACITY, "map align: more than 2^30 points in one call");
    std::vector<AlOp> aops(O);
    std::vector<int4> blk;
    std::vector<int2> chunks;
    long long n_stk[2] = {0, 0};
    for (int r = 0; r < O; ++r) {
        const ll_merge_op &o = ops[run[r]];
        AlOp &a = aops[r];
        a.chunk0 = (int)chunks.size(); a.pad = 0;
        long long nb = 0;
        for (int w = 0; w < 2; ++w) {
            const long long ns = stacks[stack_of[2 * o.src + w]].n;
            a.grid[w] = grid_of[2 * o.dst + w];
            a.blk0[w] = (int)blk.size(); a.nblk[w] = (int)((ns + LL_KNNB - 1) / LL_KNNB);
            for (long long f = 0; f < ns; f += LL_KNNB) blk.push_back(make_int4(r, w, (int)f, 0));
            n_stk[w] += ns; nb += ns;
        }
        for (long long c = 0; c * AL_CHUNK < nb; ++c) chunks.push_back(make_int2(r, (int)c));
        if (blk.size() > (size_t)INT_MAX / 2 || chunks.size() > (size_t)INT_MAX / 2) return llcms_fail(cms, LL_ERR_CAPACITY, "map align: too many stack points for one launch");
    }
    ll_ctx *ctx = llcms_map(cms, 0)->ctx;
    hipStream_t st = ctx->stream;
    AL_HIP(hipSetDevice(ctx->device));
    const size_t n_ev = 3 + 2 * (size_t)n_outer;
    while (A.ev.size() < n_ev) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return llcms_fail(cms, LL_ERR_HIP, "map align: hipEventCreate failed");
        A.ev.push_back(e);
    }
    static_assert(sizeof(ll_localize_fit) == 4 * sizeof(double), "the records lie behind the poses as 4 doubles each");
    static_assert(sizeof(ll_pose_info) == 50 * sizeof(double), "the information records lie behind the counts as 50 doubles each");
    const size_t res_doubles = (size_t)O * (7 + 4 + 1) + (info ? (size_t)O * 50 : 0);   /* poses, records, the two block counts of every op, the information records */
    int *d_T = nullptr, *d_blkcnt = nullptr, *d_blkbase = nullptr;
    float4 *d_sorted = nullptr, *d_flat = nullptr;
    double *d_res = nullptr, *d_part = nullptr, *d_lm = nullptr;
    std::vector<LLMapView> views(O);
    LLCarve W{A.d_mem};
    for (int pass = 0; pass < 2; ++pass) {                         /* first the size, then the pointers */
        W.at = 0;
        d_T = W.take<int>((size_t)n_slot * AL_TAB);
        d_sorted = W.take<float4>((size_t)n_sorted); d_flat = W.take<float4>((size_t)n_flat);
        d_blkcnt = W.take<int>(blk.size()); d_blkbase = W.take<int>(blk.size());
        d_res = W.take<double>(res_doubles); d_part = W.take<double>(chunks.size() * LL_NACC); d_lm = W.take<double>((size_t)O * LL_LM_STRIDE);
        for (int r = 0; r < O; ++r) {
            const ll_merge_op &o = ops[run[r]];
            LLMapView &M = views[r];
            std::memset(&M, 0, sizeof(M));
            size_t ns[2];
            for (int w = 0; w < 2; ++w) {
                const AlCloud &s = stacks[stack_of[2 * o.src + w]];
                ns[w] = (size_t)s.n;
                M.stk[w] = d_flat + s.first; M.n_stk[w] = (int)s.n; M.n_map[w] = (int)grids[grid_of[2 * o.dst + w]].n;
                M.ok[w] = W.take<unsigned char>(ns[w]);
                M.src[w] = W.take<int>(ns[w]);
            }
            M.qa = W.take<double>(3 * ns[0]); M.qb = W.take<double>(3 * ns[0]); M.fa = W.take<double>(3 * ns[0]); M.fb = W.take<double>(3 * ns[0]);
            M.qn = W.take<double>(3 * ns[1]); M.qd = W.take<double>(ns[1]); M.fn = W.take<double>(3 * ns[1]); M.fd = W.take<double>(ns[1]);
            M.pose = d_res + 7 * (size_t)r;
            M.counts = (int *)(d_res + (size_t)O * 11) + 2 * r;
            M.lm = d_lm + (size_t)r * LL_LM_STRIDE;
            M.huber = ctx->V.huber;
            M.row_world = 1;
        }
        if (pass == 0 && W.at > A.cap_mem) {
            void *p = nullptr;
            if (hipMalloc(&p, W.at) != hipSuccess) { (void)hipGetLastError(); return llcms_fail(cms, LL_ERR_HIP, "map align: hipMalloc failed for the workspace (" + std::to_string(W.at) + " bytes)"); }
            if (A.d_mem) (void)hipFree(A.d_mem);                    /* hipFree waits for the work that may still read it */
            A.d_mem = (unsigned char *)p; A.cap_mem = W.at;
        }
        W.p = A.d_mem;
    }
    ll_localize_fit *d_fit = (ll_localize_fit *)(d_res + (size_t)O * 7);
    ll_pose_info *d_info = (ll_pose_info *)(d_res + (size_t)O * 12);
    /* ---- the tables: segments (dst cubes first), slots, cube -> slot, ops, views, block rows, chunks, the guesses */
    std::vector<AlSeg> segs;
    std::vector<int> slot_base((size_t)n_slot), c2s(grids.size() * (size_t)CM_N, -1);
    std::vector<AlGrid> dgrids(grids.size());
    LLTiler tiles{AL_TILE};
    for (size_t g = 0; g < grids.size(); ++g) {
        const ll_cubemap *cm = llcms_map(cms, grids[g].map);
        const int w = grids[g].w;
        int base = 0, slot = grids[g].slot0;
        for (int c = 0; c < CM_N; ++c) {
            const int cnt = cm->cnt[w][c];
            if (cnt <= 0) continue;
            AlSeg s;
            s.src = cm->pool[w][cm->cur[w]] + cm->off[w][c]; s.flat = nullptr; s.cnt = cnt; s.base = base; s.at = (int)grids[g].first; s.slot = slot; s.tile0 = tiles.take(cnt);
            s.wc[0] = c % CM_W - cm->cen[0]; s.wc[1] = (c / CM_W) % CM_H - cm->cen[1]; s.wc[2] = c / (CM_W * CM_H) - cm->cen[2];
            segs.push_back(s);
            slot_base[slot] = (int)grids[g].first + base; c2s[g * CM_N + c] = slot;
            base += cnt; ++slot;
        }
        for (int k = 0; k < 3; ++k) dgrids[g].cen[k] = cm->cen[k];
        dgrids[g].pad = 0;
    }
    const unsigned long long tile_dst = tiles.next;                /* the dst cubes come first: k_al_scatter's grid */
    const size_t nseg_dst = segs.size();
    for (const AlCloud &sc : stacks) {
        const ll_cubemap *cm = llcms_map(cms, sc.map);
        int base = 0;
        for (int c = 0; c < CM_N; ++c) {
            const int cnt = cm->cnt[sc.w][c];
            if (cnt <= 0) continue;
            AlSeg s;
            s.src = cm->pool[sc.w][cm->cur[sc.w]] + cm->off[sc.w][c]; s.flat = d_flat + sc.first; s.cnt = cnt; s.base = base; s.at = 0; s.slot = -1; s.tile0 = tiles.take(cnt);
            s.wc[0] = s.wc[1] = s.wc[2] = 0;
            segs.push_back(s);
            base += cnt;
        }
    }
    if (!tiles.fits()) return llcms_fail(cms, LL_ERR_CAPACITY, "map align: too many tiles for one launch");
    llcms_begin(cms);
    const AlSeg *d_segs = (const AlSeg *)llcms_stage(cms, segs.data(), segs.size() * sizeof(AlSeg));
    const int *d_slot_base = (const int *)llcms_stage(cms, slot_base.data(), slot_base.size() * sizeof(int));
    const int *d_c2s = (const int *)llcms_stage(cms, c2s.data(), c2s.size() * sizeof(int));
    if (!d_segs || !d_slot_base || !d_c2s) return LL_ERR_HIP;
    for (size_t g = 0; g < grids.size(); ++g) dgrids[g].c2s = d_c2s + g * CM_N;
    const AlGrid *d_grids = (const AlGrid *)llcms_stage(cms, dgrids.data(), dgrids.size() * sizeof(AlGrid));
    const AlOp *d_ops = (const AlOp *)llcms_stage(cms, aops.data(), aops.size() * sizeof(AlOp));
    const LLMapView *d_views = (const LLMapView *)llcms_stage(cms, views.data(), views.size() * sizeof(LLMapView));
    const int4 *d_blk = blk.empty() ? nullptr : (const int4 *)llcms_stage(cms, blk.data(), blk.size() * sizeof(int4));
    const int2 *d_chunks = chunks.empty() ? nullptr : (const int2 *)llcms_stage(cms, chunks.data(), chunks.size() * sizeof(int2));
    if (!d_grids || !d_ops || !d_views || (!blk.empty() && !d_blk) || (!chunks.empty() && !d_chunks)) return LL_ERR_HIP;
    {
        std::vector<double> res(res_doubles, 0.0);
        for (int r = 0; r < O; ++r) std::memcpy(res.data() + 7 * (size_t)r, ops[run[r]].T_w7, 7 * sizeof(double));
        if (!llcms_stage_to(cms, res.data(), res.size() * sizeof(double), d_res)) return LL_ERR_HIP;
    }
    /* ---- build */
    size_t e = 0;
    AL_HIP(hipEventRecord(A.ev[e++], st));
    AL_HIP(hipMemsetAsync(d_T, 0, (size_t)n_slot * AL_TAB * sizeof(int), st));
    hipLaunchKernelGGL(k_al_count, dim3((unsigned)tiles.next), dim3(256), 0, st, d_segs, (int)segs.size(), d_T);
    hipLaunchKernelGGL(k_al_scan, dim3((unsigned)n_slot), dim3(256), 0, st, d_T, d_slot_base);
    hipLaunchKernelGGL(k_al_scatter, dim3((unsigned)tile_dst), dim3(256), 0, st, d_segs, (int)nseg_dst, d_T, d_sorted);
    AL_HIP(hipEventRecord(A.ev[e++], st));
    /* ---- n_outer x {search + fit, blocks, 1 + max_num_iterations x (evaluate, solve)}, enqueued back to back */
    const LLLmOpt lo = ll_to_dev_opt(opt);
    auto associate = [&]() {
        if (!blk.empty()) hipLaunchKernelGGL(k_al_knn, dim3((unsigned)blk.size()), dim3(LL_KNNB), 0, st, d_views, d_ops, d_grids, d_blk, (const int *)d_T, (const float4 *)d_sorted, d_blkcnt);
        hipLaunchKernelGGL(k_al_cscan, dim3(2 * O), dim3(256), 0, st, d_views, d_ops, (const int *)d_blkcnt, d_blkbase);
        if (!blk.empty()) hipLaunchKernelGGL(k_al_place, dim3((unsigned)blk.size()), dim3(LL_KNNB), 0, st, d_views, d_blk, (const int *)d_blkbase);
    };
    for (int it = 0; it < n_outer; ++it) {
        associate();
        AL_HIP(hipEventRecord(A.ev[e++], st));
        for (int round = 0; round <= lo.max_num_iterations; ++round) {
            if (!chunks.empty()) hipLaunchKernelGGL(k_al_eval<false>, dim3((unsigned)chunks.size()), dim3(256), 0, st, d_views, d_chunks, d_part);
            hipLaunchKernelGGL(k_al_solve, dim3(O), dim3(64), 0, st, d_views, d_ops, (const double *)d_part, lo, round);
        }
        AL_HIP(hipEventRecord(A.ev[e++], st));
    }
    if (fit || info) {                                             /* the blocks at the final pose, reduced */
        associate();
        if (!chunks.empty()) hipLaunchKernelGGL(k_al_eval<true>, dim3((unsigned)chunks.size()), dim3(256), 0, st, d_views, d_chunks, d_part);
        hipLaunchKernelGGL(k_al_fitsum, dim3(O), dim3(64), 0, st, d_views, d_ops, (const double *)d_part, d_fit);
    }
    if (info) {                                                    /* the same blocks' normal equations; the partials are free again */
        if (!chunks.empty()) hipLaunchKernelGGL(k_al_eval<false>, dim3((unsigned)chunks.size()), dim3(256), 0, st, d_views, d_chunks, d_part);
        hipLaunchKernelGGL(k_al_infosum, dim3(O), dim3(64), 0, st, d_views, d_ops, (const double *)d_part, (const ll_localize_fit *)d_fit, d_info);
    }
    AL_HIP(hipEventRecord(A.ev[e++], st));
    AL_HIP(hipGetLastError());
    /* ---- the ONE synchronisation: poses, records, block counts */
    double *pin = (double *)ll_pinned_scratch(res_doubles * sizeof(double));
    if (!pin) return llcms_fail(cms, LL_ERR_HIP, "map align: no page-locked scratch");
    AL_HIP(hipMemcpyAsync(pin, d_res, res_doubles * sizeof(double), hipMemcpyDeviceToHost, st));
    const int rc = llcms_sync(cms); if (rc) return rc;
    auto span = [&](size_t a, size_t b) { return ll_event_ms(A.ev[a], A.ev[b], 0.0); };
    A.ms[0] = span(0, 1);
    for (int it = 0; it < n_outer; ++it) { A.ms[1] += span(1 + 2 * (size_t)it, 2 + 2 * (size_t)it); A.ms[2] += span(2 + 2 * (size_t)it, 3 + 2 * (size_t)it); }
    A.ms[3] = span(1 + 2 * (size_t)n_outer, 2 + 2 * (size_t)n_outer);
    A.counts[0] = n_stk[0] + n_stk[1]; A.counts[1] = n_sorted;
    const int *cnt = (const int *)(pin + (size_t)O * 11);
    int bad = -1;
    for (int r = 0; r < O; ++r) {
        const int i = run[r];
        bool nan = false;
        for (int k = 0; k < 7; ++k) nan = nan || std::isnan(pin[7 * (size_t)r + k]);
        std::memcpy(T_w7 + 7 * i, pin + 7 * (size_t)r, 7 * sizeof(double));
        if (fit) std::memcpy(fit + i, pin + (size_t)O * 7 + 4 * (size_t)r, sizeof(ll_localize_fit));
        if (info) std::memcpy(info + i, pin + (size_t)O * 12 + 50 * (size_t)r, sizeof(ll_pose_info));
        if (ran) ran[i] = !nan;
        if (nan && bad < 0) bad = i;
        if (n_outer > 0 || fit || info) A.counts[2] += (long long)cnt[2 * r] + cnt[2 * r + 1];
    }
    if (bad >= 0) return llcms_fail(cms, LL_ERR_STATE, "map align: op " + std::to_string(bad) + ": the solve returned an undefined pose (NaN)");
    return LL_OK;
}

/* the last ll_cubemaps_align: ms4 = build, search + fit, evaluate + solve, fit record (device events); counts3 = stack points,
 * map points, residual blocks at the end */
extern "C" int ll_cubemaps_align_timing(const ll_cubemaps *cms, double *ms4, long long *counts3)
{
    if (!cms) return LL_ERR_ARG;
    const LLMapAlign &A = llcms_align_state(const_cast<ll_cubemaps *>(cms));
    if (ms4) for (int k = 0; k < 4; ++k) ms4[k] = A.ms[k];
    if (counts3) for (int k = 0; k < 3; ++k) counts3[k] = A.counts[k];
    return LL_OK;
}
