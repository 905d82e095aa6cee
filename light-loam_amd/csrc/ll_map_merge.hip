/*
 * ll_map_merge.hip -- cube maps of one ll_cubemaps combined on the device: op (dst, src, T) takes every point of map src through
 * pointAssociateToMap (laserMapping.cpp:125-134) with the pose T, bins it with dst's centre (:2108-2125) and appends it to the cube
 * it falls into; every cube that received a point is then down-sized by the library's VoxelGrid (:2151-2165), as a mapping frame
 * does with its valid cubes.  The update path of ll_cubemaps.hip is sized for one scan (max_scan_*, cap_work); a merge moves whole
 * maps from a pool to a pool, so it has its own kernels and its own workspace, grown to the need of the call.
 *
 * One record per (op, cloud type).  The points of a record are numbered in the order an LL_MAP_ALL export lists that type: cube
 * 0 .. 4850 of src, inside a cube its own order; the records lie back to back in one flat index space.
 *   k_mm_assign   a workgroup takes one tile of one source cloud where it lies in src's pool (a segment table and a binary search
 *                 over the segments' first tiles, as k_map_export): transformed point and cube key per point, and the points per
 *                 (record, cube) with one add per wave and cube -- nearly all points of a source cube land in at most eight
 *                 destination cubes.  Key 4851 = outside the array (dropped, counted in the same table).
 *   k_mm_cstart   per record the exclusive scan of the 4852 counts: where each cube's new points begin in the by-cube order.
 *   k_mm_hist     a counting sort over the 4852 bins, stable and the same from run to run: the record's points in chunks of 2048,
 *                 one LDS histogram per chunk;
 *   k_mm_colscan  per (record, cube) the running sum over the record's chunks, from the cube's beginning;
 *   k_mm_place    one wave per chunk walks it in order: a point's place is its chunk's start for its cube plus the points of the
 *                 same cube before it in the chunk (ballots inside the wave, a counter per cube in LDS).  No rank comes from the
 *                 order in which an atomic is served.
 *   k_mm_gather   copies over a table in fixed tiles (k_map_export's shape), optionally through an index: the filter input --
 *                 per touched cube its old cloud, then its new points in order -- and, after the filters, the commit copy.
 * The host synchronises three times per call whatever the number of ops: the per-cube counts, the filtered sizes, the commit;
 * plus the voxel filter's read-back when a filter call is above 65 536 points and cannot sort inside its workgroups.
 *
 * ll_cubemaps_insert_keyframes (a map rebuilt or extended from the frames of an ll_keyframes store, each frame under its own pose) is
 * the same machine with the source and the transform per frame: k_kf_assign is k_mm_assign over the (frame, type) clouds where they
 * lie in the store's pool, with a pose per SEGMENT; a record's flat order is its listed frames back to back.  Everything from
 * k_mm_cstart to the commit is mm_run, which both entry points call; an op may ask for its dst to be emptied first, which mm_run
 * does once the capacity decision has passed and takes back if the call fails before its commit.
 *
 * ll_cubemaps_insert_keyframes_filtered is the same call with k_kf_assign<true>: a point that the rule removes by its two visibility
 * counters (ll_visibility.hip; read at the point's pool index) gets key 4851 like a point outside the array, and the removed points
 * per record are counted behind the count tables -- so everything from k_mm_cstart on is untouched, and `dropped` is the outside
 * bin minus the removed ones.
 */
#include "ll_cubemaps.h"
#include "ll_keyframes.h"
#include "ll_tiles.h"
#include <chrono>
#include <climits>
#include <cmath>
#include <functional>
#include <numeric>

#define MM_BINS (CM_N + 1)               /* 4851 cubes + "outside the array" */
#define MM_CHUNK 2048                    /* points per histogram row of the counting sort */
#define MM_TILE 1024                     /* points per workgroup of k_mm_assign / k_mm_gather: 256 lanes x 4 */

struct MmRec { double T[7]; int cen[3]; int first, n, chunk0, nchunk, pad; };      /* first: its first point in the flat order */
struct MmSeg { const float4 *src; int dst, cnt; unsigned tile0; int rec; };        /* one source cloud; dst: flat index of its first point */
struct KfSeg { const float4 *src; int dst, cnt; unsigned tile0; int rec; double T[7]; };   /* keyframe insert: one (frame, type) cloud and that frame's pose */
struct MmChunk { int first, cnt, rec, pad; };
struct MmCopy { const float4 *src; const int *index; float4 *dst; int cnt; unsigned tile0; };   /* dst[i] = index ? src[index[i]] : src[i] */

/* ------------------------------------------------------------------ kernels */
/* the filtered keyframe insert: the store's pool, the visibility counters (two bytes per pool point: through, hit), the rule, and
 * removed[record] */
struct KfFilter { const float4 *pool; const unsigned char *vis; int min_through, max_hit; int *removed; };

/* tile `tile` of a source cloud of cnt points whose first point has the flat index dst, under the pose Tsrc and the centre of record rec.
 * FILTER: a point the rule removes (through >= min_through && hit <= max_hit, its counters at its pool index) gets the "outside
 * the array" key like a dropped point and is counted in removed[rec] with one add per wave */
template <bool FILTER>
__device__ __forceinline__ void mm_assign_tile(const float4 *src, int dst, int cnt, int tile, const double *Tsrc, const MmRec *recs, int rec, float4 *tp, int *keys, int *addcnt,
                                               const KfFilter *F = nullptr)
{
    const MmRec &R = recs[rec];
    const int first = tile * MM_TILE, n = min(MM_TILE, cnt - first);
    double T[7]; int cen[3];                                      /* like the points: every load before the first store */
    for (int k = 0; k < 7; ++k) T[k] = Tsrc[k];
    for (int k = 0; k < 3; ++k) cen[k] = R.cen[k];
    int *count = addcnt + (size_t)rec * MM_BINS;
    float4 po[MM_TILE / 256];
#pragma unroll
    for (int k = 0; k < MM_TILE / 256; ++k) po[k] = src[first + min(k * 256 + (int)threadIdx.x, n - 1)];   /* every load before the first store */
    bool gone[MM_TILE / 256] = {};
    if (FILTER) {
        const uchar2 *vis = (const uchar2 *)F->vis + (src - F->pool) + first;
        int n_gone = 0;
#pragma unroll
        for (int k = 0; k < MM_TILE / 256; ++k) {
            const int i = k * 256 + (int)threadIdx.x;
            const uchar2 th = vis[min(i, n - 1)];
            gone[k] = i < n && (int)th.x >= F->min_through && (int)th.y <= F->max_hit;
            n_gone += __popcll(__ballot(gone[k]));
        }
        if ((threadIdx.x & 63) == 0 && n_gone > 0) atomicAdd(&F->removed[rec], n_gone);
    }
#pragma unroll
    for (int k = 0; k < MM_TILE / 256; ++k) {
        const int i = k * 256 + (int)threadIdx.x;
        int cube = -1;                                            /* -1: no point */
        if (i < n) {
            /* pointAssociateToMap (:125-134) and the cube (:2108-2125) as a frame's update has them (ll_map_to_world, cm_cube_of); the
             * pose is used as given, never normalised */
            float sx, sy, sz;
            ll_map_to_world(T, po[k], sx, sy, sz);
            tp[dst + first + i] = make_float4(sx, sy, sz, po[k].w);
            int ci, cj, ck;
            cube = cm_cube_of(sx, sy, sz, cen, &ci, &cj, &ck);
            if (cube < 0) cube = CM_N;                            /* outside the array: a bin of its own */
            if (FILTER && gone[k]) cube = CM_N;                   /* removed: the same bin, told apart by removed[rec] */
            keys[dst + first + i] = cube;
        }
        cm_wave_count(cube, count);                               /* one add per wave and cube */
    }
}

__global__ __launch_bounds__(256) void k_mm_assign(const MmSeg *seg, int nseg, const MmRec *recs, float4 *tp, int *keys, int *addcnt)
{
    const MmSeg s = seg[ll_tile_find(seg, nseg, blockIdx.x)];
    mm_assign_tile<false>(s.src, s.dst, s.cnt, (int)(blockIdx.x - s.tile0), recs[s.rec].T, recs, s.rec, tp, keys, addcnt);
}

/* keyframe insert: the same for one tile of one (frame, type) cloud where it lies in the store's pool; the pose is its SEGMENT's --
 * every listed frame has its own -- and the record (op, type) gives the centre and the count table.  A record's flat order is its
 * frames back to back, so the chunks of the counting sort below run across frame boundaries.  FILTER = false is the plain insert
 * (F is not read); FILTER = true is ll_cubemaps_insert_keyframes_filtered */
template <bool FILTER>
__global__ __launch_bounds__(256) void k_kf_assign(const KfSeg *seg, int nseg, const MmRec *recs, float4 *tp, int *keys, int *addcnt, KfFilter F)
{
    const KfSeg *s = seg + ll_tile_find(seg, nseg, blockIdx.x);
    mm_assign_tile<FILTER>(s->src, s->dst, s->cnt, (int)(blockIdx.x - s->tile0), s->T, recs, s->rec, tp, keys, addcnt, &F);
}

/* cstart[r][b] = addcnt[r][0] + .. + addcnt[r][b - 1]: one workgroup per record */
__global__ __launch_bounds__(256) void k_mm_cstart(const int *addcnt, int *cstart)
{
    __shared__ int sc[4];
    const int *a = addcnt + (size_t)blockIdx.x * MM_BINS;
    int *c = cstart + (size_t)blockIdx.x * MM_BINS;
    int base = 0;
    for (int b0 = 0; b0 < MM_BINS; b0 += 256) {
        const int b = b0 + (int)threadIdx.x;
        int total;
        const int pos = base + ll_block_exscan_n<4>(b < MM_BINS ? a[b] : 0, sc, total);
        if (b < MM_BINS) c[b] = pos;
        base += total;
    }
}

__global__ __launch_bounds__(256) void k_mm_hist(const MmChunk *chunks, const int *keys, int *H)
{
    __shared__ int h[MM_BINS];
    const MmChunk c = chunks[blockIdx.x];
    for (int b = threadIdx.x; b < MM_BINS; b += 256) h[b] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < c.cnt; i += 256) atomicAdd(&h[keys[c.first + i]], 1);
    __syncthreads();
    int *row = H + (size_t)blockIdx.x * MM_BINS;
    for (int b = threadIdx.x; b < MM_BINS; b += 256) row[b] = h[b];
}

/* H[chunk][b]: the count of cube b in the chunk -> the place of the chunk's first point of cube b in the record's by-cube order */
__global__ __launch_bounds__(256) void k_mm_colscan(const MmRec *recs, const int *cstart, int *H)
{
    const int b = blockIdx.x * 256 + (int)threadIdx.x;
    if (b >= MM_BINS) return;
    const MmRec &R = recs[blockIdx.y];
    int run = cstart[(size_t)blockIdx.y * MM_BINS + b];
    int *col = H + (size_t)R.chunk0 * MM_BINS + b;
    for (int k0 = 0; k0 < R.nchunk; k0 += 8) {
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = k0 + j < R.nchunk ? col[(size_t)(k0 + j) * MM_BINS] : 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) if (k0 + j < R.nchunk) { col[(size_t)(k0 + j) * MM_BINS] = run; run += v[j]; }
    }
}

/* one wave per chunk, in order: perm[record's first + place] = flat index of the point */
__global__ __launch_bounds__(64) void k_mm_place(const MmChunk *chunks, const MmRec *recs, const int *keys, const int *H, int *perm)
{
    __shared__ int pos[MM_BINS];
    const MmChunk c = chunks[blockIdx.x];
    const int lane = threadIdx.x, rec_first = recs[c.rec].first;
    const int *row = H + (size_t)blockIdx.x * MM_BINS;
    for (int b = lane; b < MM_BINS; b += 64) pos[b] = row[b];
    __syncthreads();
    for (int i0 = 0; i0 < c.cnt; i0 += 64) {
        const int i = i0 + lane;
        const int key = i < c.cnt ? keys[c.first + i] : -1;
        int place = 0;
        unsigned long long todo = __ballot(key >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int k0 = __shfl(key, leader);
            const unsigned long long same = __ballot(key == k0);
            int base = 0;
            if (lane == leader) { base = pos[k0]; pos[k0] = base + __popcll(same); }
            base = __shfl(base, leader);
            if (key == k0) place = base + __popcll(same & ((1ull << lane) - 1ull));
            todo &= ~same;
        }
        if (key >= 0) perm[rec_first + place] = c.first + i;
        __syncthreads();                                          /* one wave: the counters of this step before the next step reads them */
    }
}

__global__ __launch_bounds__(256) void k_mm_gather(const MmCopy *ops, int nops)
{
    const MmCopy o = ops[ll_tile_find(ops, nops, blockIdx.x)];
    const int first = (int)(blockIdx.x - o.tile0) * MM_TILE, n = min(MM_TILE, o.cnt - first);
    const ll_gf4 *src = (const ll_gf4 *)o.src;
    ll_gf4 *dst = (ll_gf4 *)o.dst + first;
    ll_f4 v[MM_TILE / 256];
    if (o.index) {
        int idx[MM_TILE / 256];
#pragma unroll
        for (int k = 0; k < MM_TILE / 256; ++k) idx[k] = o.index[first + min(k * 256 + (int)threadIdx.x, n - 1)];
#pragma unroll
        for (int k = 0; k < MM_TILE / 256; ++k) v[k] = src[idx[k]];
    } else {
#pragma unroll
        for (int k = 0; k < MM_TILE / 256; ++k) v[k] = src[first + min(k * 256 + (int)threadIdx.x, n - 1)];
    }
#pragma unroll
    for (int k = 0; k < MM_TILE / 256; ++k) { const int i = k * 256 + (int)threadIdx.x; if (i < n) dst[i] = v[k]; }
}

/* ------------------------------------------------------------------ host side */
void llmm_free(LLMapMerge &G)
{
    for (int k = 0; k < 2; ++k) if (G.d_mem[k]) (void)hipFree(G.d_mem[k]);
    if (G.have_ev) for (int k = 0; k < LL_MM_EVENTS; ++k) (void)hipEventDestroy(G.ev[k]);
    G = LLMapMerge();
}

/* buffer k (0: the by-cube order, sized from the source maps; 1: the filters, sized from what they receive) grown to `bytes`; the
 * old buffer is kept when the new one cannot be had */
static unsigned char *mm_reserve(LLMapMerge &G, int k, size_t bytes, std::string &err)
{
    if (bytes > G.cap_mem[k]) {
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            err = "map merge: hipMalloc failed for the workspace (" + std::to_string(bytes) + " bytes)"; return nullptr;
        }
        if (G.d_mem[k]) (void)hipFree(G.d_mem[k]);                  /* hipFree waits for the work that may still read it */
        G.d_mem[k] = (unsigned char *)p; G.cap_mem[k] = bytes;
    }
    return G.d_mem[k];
}

static const char *mm_type(int w) { return w ? "surf" : "corner"; }

#define MM_HIP(call) LL_HIP_CHECK(llcms_fail, cms, J.what, call, #call)

static int mm_gather(ll_cubemaps *cms, const std::string &what, std::vector<MmCopy> &ops, hipStream_t st)
{
    LLTiler T{MM_TILE};
    for (MmCopy &o : ops) o.tile0 = T.take(o.cnt);
    if (ops.empty()) return LL_OK;
    if (!T.fits()) return llcms_fail(cms, LL_ERR_CAPACITY, what + "too many tiles for one launch");
    const MmCopy *d = (const MmCopy *)llcms_stage(cms, ops.data(), ops.size() * sizeof(MmCopy));
    if (!d) return LL_ERR_HIP;
    hipLaunchKernelGGL(k_mm_gather, dim3((unsigned)T.next), dim3(256), 0, st, d, (int)ops.size());
    return LL_OK;
}

/* what ll_cubemaps_merge and ll_cubemaps_insert_keyframes hand to the stages they share: per op its dst map, whether dst is first
 * emptied (reset, with the centre cen: keyframe insert only) and how last_error names the op; the records (one per (op, type), their
 * points back to back in one flat index space of N points) and the chunks of the counting sort; `assign`, which stages the
 * caller's own segment table (`stage`) and launches its assign kernel over d_recs into tp / keys / addcnt; where the call's figures go */
struct MmOp { int dst, reset, cen[3]; std::string who; };
struct MmJob {
    std::string what;                                             /* "map merge: " */
    std::vector<MmOp> ops;
    std::vector<MmRec> recs;
    std::vector<MmChunk> chunks;
    long long N = 0;
    std::function<bool()> stage;                                  /* the caller's segment table into the call's arena; false: failed */
    std::function<void(const MmRec *d_recs, float4 *d_tp, int *d_keys, int *d_addcnt, hipStream_t st)> assign;
    bool filtered = false;                                        /* the assign stage also counts removed points: nrec ints behind the count tables */
    double *ms = nullptr; long long *counts = nullptr;            /* [4], [3] of LLMapMerge */
};

/* a reset made once the capacity decision has passed is taken back when the call fails before its commit: the tables and the
 * per-frame counts as they were (no pool has been written by then) */
struct MmUndo {
    struct Saved { ll_cubemap *cm; CmTables t; int n_map[2], n_stk[2]; bool broken, has_frame; };
    std::vector<Saved> saved;
    void keep(ll_cubemap *cm) { saved.push_back({cm, *cm, {cm->map->M.n_map[0], cm->map->M.n_map[1]}, {cm->map->M.n_stk[0], cm->map->M.n_stk[1]}, cm->broken, cm->has_frame}); }
    void done() { saved.clear(); }
    ~MmUndo()
    {
        for (Saved &s : saved) {
            static_cast<CmTables &>(*s.cm) = s.t;
            for (int w = 0; w < 2; ++w) { s.cm->map->M.n_map[w] = s.n_map[w]; s.cm->map->M.n_stk[w] = s.n_stk[w]; }
            s.cm->broken = s.broken; s.cm->has_frame = s.has_frame;
        }
    }
};

static void mm_reset(ll_cubemaps *cms, const MmOp &o)
{
    (void)ll_cubemaps_reset(cms, o.dst);
    for (int k = 0; k < 3; ++k) llcms_map(cms, o.dst)->cen[k] = o.cen[k];
}

/* everything after the refusals that need no look at a point: workspace, the assign stage, then from k_mm_cstart to the commit --
 * count read-back, capacity decision, plan, gather, filter, commit */
static int mm_run(ll_cubemaps *cms, MmJob &J, long long *added, long long *dropped, long long *removed = nullptr)
{
    LLMapMerge &G = llcms_merge_state(cms);
    ll_ctx *ctx = llcms_map(cms, 0)->ctx;
    hipStream_t st = ctx->stream;
    const int n_ops = (int)J.ops.size(), nrec = 2 * n_ops;
    const std::vector<MmRec> &recs = J.recs;
    const std::vector<MmChunk> &chunks = J.chunks;
    const long long N = J.N;
    J.ms[0] = J.ms[1] = J.ms[2] = J.ms[3] = 0.0; J.counts[0] = N; J.counts[1] = J.counts[2] = 0;
    if (added) std::fill(added, added + nrec, 0ll);
    if (dropped) std::fill(dropped, dropped + nrec, 0ll);
    if (removed) std::fill(removed, removed + nrec, 0ll);
    if (N == 0) {                                                 /* empty sources: nothing to move */
        for (const MmOp &o : J.ops) if (o.reset) mm_reset(cms, o);
        return LL_OK;
    }
    MM_HIP(hipSetDevice(ctx->device));
    if (!G.have_ev) {
        for (int k = 0; k < LL_MM_EVENTS; ++k)
            if (hipEventCreate(&G.ev[k]) != hipSuccess) { for (int j = 0; j < k; ++j) (void)hipEventDestroy(G.ev[j]); return llcms_fail(cms, LL_ERR_HIP, J.what + "hipEventCreate failed"); }
        G.have_ev = true;
    }
    LLCarve A{nullptr};                                           /* first the size, then the pointers */
    A.take<float4>((size_t)N); A.take<int>((size_t)N); A.take<int>((size_t)N);
    const size_t n_cnt = (size_t)nrec * MM_BINS + (J.filtered ? (size_t)nrec : 0);
    A.take<int>(n_cnt); A.take<int>((size_t)nrec * MM_BINS); A.take<int>(chunks.size() * MM_BINS);
    {
        std::string why;
        A.p = mm_reserve(G, 0, A.at, why);
        if (!A.p) return llcms_fail(cms, LL_ERR_HIP, why);
    }
    A.at = 0;
    float4 *d_tp = A.take<float4>((size_t)N);
    int *d_keys = A.take<int>((size_t)N), *d_perm = A.take<int>((size_t)N);
    int *d_addcnt = A.take<int>(n_cnt), *d_cstart = A.take<int>((size_t)nrec * MM_BINS), *d_H = A.take<int>(chunks.size() * MM_BINS);
    llcms_begin(cms);
    const MmRec *d_recs = (const MmRec *)llcms_stage(cms, recs.data(), recs.size() * sizeof(MmRec));
    const MmChunk *d_chunks = (const MmChunk *)llcms_stage(cms, chunks.data(), chunks.size() * sizeof(MmChunk));
    if (!d_recs || !d_chunks || !J.stage()) return LL_ERR_HIP;
    /* ---- stage A: points -> cubes, by-cube order; host: the cubes' new-point counts of every record */
    MM_HIP(hipMemsetAsync(d_addcnt, 0, n_cnt * sizeof(int), st));
    MM_HIP(hipEventRecord(G.ev[0], st));
    J.assign(d_recs, d_tp, d_keys, d_addcnt, st);
    MM_HIP(hipEventRecord(G.ev[1], st));
    hipLaunchKernelGGL(k_mm_cstart, dim3(nrec), dim3(256), 0, st, (const int *)d_addcnt, d_cstart);
    hipLaunchKernelGGL(k_mm_hist, dim3((unsigned)chunks.size()), dim3(256), 0, st, d_chunks, (const int *)d_keys, d_H);
    hipLaunchKernelGGL(k_mm_colscan, dim3((MM_BINS + 255) / 256, nrec), dim3(256), 0, st, d_recs, (const int *)d_cstart, d_H);
    hipLaunchKernelGGL(k_mm_place, dim3((unsigned)chunks.size()), dim3(64), 0, st, d_chunks, d_recs, (const int *)d_keys, (const int *)d_H, d_perm);
    MM_HIP(hipEventRecord(G.ev[2], st));
    MM_HIP(hipGetLastError());
    std::vector<int> addcnt(n_cnt);
    {
        int *pin = (int *)ll_pinned_scratch(addcnt.size() * sizeof(int));
        if (!pin) return llcms_fail(cms, LL_ERR_HIP, J.what + "no page-locked scratch");
        MM_HIP(hipMemcpyAsync(pin, d_addcnt, addcnt.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        const int rc = llcms_sync(cms); if (rc) return rc;
        std::memcpy(addcnt.data(), pin, addcnt.size() * sizeof(int));
    }
    /* ---- will it fit?  Every op and both types, before any pair table changes: a dst pool must hold what the map holds of the
     * type (nothing, when the op resets it) plus the added points, so that the commit below cannot fail whatever the filters leave */
    std::vector<long long> n_add(nrec, 0);
    long long bound[2] = {0, 0};
    bool any_reset = false;
    for (int r = 0; r < nrec; ++r) {
        const int *a = addcnt.data() + (size_t)r * MM_BINS;
        const MmOp &o = J.ops[r / 2];
        const ll_cubemap *dst = llcms_map(cms, o.dst);
        const int w = r & 1;
        long long live = 0;
        for (int c = 0; c < CM_N; ++c) { n_add[r] += a[c]; if (!o.reset) live += dst->cnt[w][c]; }
        if (added) added[r] = n_add[r];
        const int gone = J.filtered ? addcnt[(size_t)nrec * MM_BINS + r] : 0;     /* removed points sit in the outside bin too */
        if (dropped) dropped[r] = a[CM_N] - gone;
        if (removed) removed[r] = gone;
        if (live + n_add[r] > (long long)dst->cap_pool)
            return llcms_fail(cms, LL_ERR_CAPACITY, J.what + "op " + std::to_string(r / 2) + " (" + o.who + "): " +
                              std::to_string(live) + " " + mm_type(w) + " points + " + std::to_string(n_add[r]) + " added, pool_points is " + std::to_string(dst->cap_pool));
        bound[w] += live + n_add[r]; any_reset = any_reset || o.reset;
    }
    MmUndo undo;
    if (any_reset) {                                              /* the filter call's own limit (below), decided while nothing has changed */
        for (int w = 0; w < 2; ++w)
            if (bound[w] > (long long)(INT_MAX / 2)) return llcms_fail(cms, LL_ERR_CAPACITY, J.what + "the touched " + mm_type(w) + " cubes hold more points than one filter call takes");
        for (const MmOp &o : J.ops) if (o.reset) { undo.keep(llcms_map(cms, o.dst)); mm_reset(cms, o); }
    }
    /* ---- stage B: one voxel-grid segment per touched cube of every op -- its cloud, then its new points in order */
    std::vector<CmPlan> plan(nrec);
    std::vector<std::vector<int>> touched(nrec);
    std::vector<int> seg_off[2] = {std::vector<int>(1, 0), std::vector<int>(1, 0)}, seg0(nrec, 0);
    long long F[2] = {0, 0};
    for (int w = 0; w < 2; ++w) {
        for (int i = 0; i < n_ops; ++i) {
            const int r = 2 * i + w;
            const int *a = addcnt.data() + (size_t)r * MM_BINS;
            for (int c = 0; c < CM_N; ++c) if (a[c] > 0) touched[r].push_back(c);
            plan[r] = cm_plan(*llcms_map(cms, J.ops[i].dst), w, touched[r].data(), (int)touched[r].size(), a);
            seg0[r] = (int)seg_off[w].size() - 1;
            for (size_t s = 1; s < plan[r].seg_off.size(); ++s) seg_off[w].push_back((int)(F[w] + plan[r].seg_off[s]));
            F[w] += plan[r].seg_off.back();
        }
        if (F[w] > (long long)(INT_MAX / 2)) return llcms_fail(cms, LL_ERR_CAPACITY, J.what + "the touched " + mm_type(w) + " cubes hold more points than one filter call takes");
    }
    const size_t nseg[2] = {seg_off[0].size() - 1, seg_off[1].size() - 1};
    J.counts[1] = (long long)(nseg[0] + nseg[1]);
    float4 *d_work[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};
    int *d_nout = nullptr;
    LLVoxWork W[2];
    {
        LLCarve B{nullptr};
        unsigned char *vox[2] = {nullptr, nullptr};
        for (int pass = 0; pass < 2; ++pass) {
            B.at = 0;
            d_nout = B.take<int>(4);
            for (int w = 0; w < 2; ++w) {
                d_work[w] = B.take<float4>((size_t)F[w]); d_out[w] = B.take<float4>((size_t)F[w]);
                vox[w] = B.take<unsigned char>(ll_vox_work_bytes((int)F[w], (int)nseg[w] + 1));
            }
            if (pass == 0) {
                std::string why;
                B.p = mm_reserve(G, 1, B.at, why);
                if (!B.p) return llcms_fail(cms, LL_ERR_HIP, why);
            }
        }
        for (int w = 0; w < 2; ++w) ll_vox_work_carve(vox[w], (int)F[w], (int)nseg[w] + 1, &W[w]);
    }
    std::vector<MmCopy> cp;
    for (int w = 0; w < 2; ++w)
        for (int i = 0; i < n_ops; ++i) {
            const int r = 2 * i + w;
            const ll_cubemap *dst = llcms_map(cms, J.ops[i].dst);
            for (const CmPiece &e : plan[r].pieces) {             /* the new points of a cube in the record's by-cube order */
                float4 *at = d_work[w] + seg_off[w][seg0[r]] + e.dst;
                if (e.old_cnt > 0) cp.push_back({dst->pool[w][dst->cur[w]] + e.old_off, nullptr, at, e.old_cnt, 0});
                cp.push_back({d_tp, d_perm + recs[r].first + e.new_first, at + e.old_cnt, e.new_cnt, 0});
            }
        }
    MM_HIP(hipEventRecord(G.ev[3], st));
    int rc = mm_gather(cms, J.what, cp, st); if (rc) return rc;
    MM_HIP(hipEventRecord(G.ev[4], st));
    for (int w = 0; w < 2; ++w) {
        if (F[w] <= 0) continue;
        const int max_seg = nseg[w] > 1 ? cm_max_segment(seg_off[w]) : 0;
        if (!llcms_stage_to(cms, seg_off[w].data(), seg_off[w].size() * sizeof(int), W[w].seg_off)) return LL_ERR_HIP;
        /* the voxel filter's sort reads back once when it cannot stay inside the workgroups (ll_voxel.hip): counted with the syncs */
        if (ll_voxel_grid_segments_reads_back((int)F[w], (int)nseg[w], max_seg)) llcms_count_sync(cms);
        if (ll_voxel_grid_segments(d_work[w], (int)F[w], (int)nseg[w], llcms_leaf(cms)[w], W[w], d_out[w], d_nout + w, st, max_seg))
            return llcms_fail(cms, LL_ERR_HIP, J.what + "voxel filter: read-back failed");
    }
    MM_HIP(hipEventRecord(G.ev[5], st));
    MM_HIP(hipGetLastError());
    std::vector<int> seg_count[2];
    {
        const size_t n0 = nseg[0], n1 = nseg[1];
        int *pin = (int *)ll_pinned_scratch((n0 + n1 + 2) * sizeof(int));
        if (!pin) return llcms_fail(cms, LL_ERR_HIP, J.what + "no page-locked scratch");
        if (n0) MM_HIP(hipMemcpyAsync(pin, W[0].seg_count, n0 * sizeof(int), hipMemcpyDeviceToHost, st));
        if (n1) MM_HIP(hipMemcpyAsync(pin + n0, W[1].seg_count, n1 * sizeof(int), hipMemcpyDeviceToHost, st));
        rc = llcms_sync(cms); if (rc) return rc;
        seg_count[0].assign(pin, pin + n0); seg_count[1].assign(pin + n0, pin + n0 + n1);
    }
    /* ---- commit: from here on a failure leaves the pair tables half-updated (the dst maps are marked unusable).  The capacity
     * decision above covers it: the filtered clouds are never larger than what went into the filters */
    undo.done();
    for (int i = 0; i < n_ops; ++i) llcms_map(cms, J.ops[i].dst)->broken = true;
    cp.clear();
    long long n_out_all = 0;
    for (int w = 0; w < 2; ++w) {
        size_t out_at = 0;
        for (int i = 0; i < n_ops; ++i) {
            const int r = 2 * i + w, n_set = (int)touched[r].size(), *sc = seg_count[w].data() + seg0[r];
            if (n_set == 0) continue;
            ll_cubemap *dst = llcms_map(cms, J.ops[i].dst);
            const size_t n = std::accumulate(sc, sc + n_set, (size_t)0);        /* nothing grows outside the set: this is all the pool takes */
            const CmCommit K = cm_commit(*dst, w, plan[r], touched[r].data(), n_set, addcnt.data() + (size_t)r * MM_BINS, sc, n);
            cm_run_moves(dst, w, K.moves);                        /* a compaction: launched at once, the copies below follow it */
            if (n > 0) cp.push_back({d_out[w] + out_at, nullptr, dst->pool[w][dst->cur[w]] + K.at, (int)n, 0});
            out_at += n; n_out_all += (long long)n;
        }
    }
    MM_HIP(hipEventRecord(G.ev[6], st));
    rc = mm_gather(cms, J.what, cp, st); if (rc) return rc;      /* after every compaction above: stream order */
    MM_HIP(hipEventRecord(G.ev[7], st));
    MM_HIP(hipGetLastError());
    rc = llcms_sync(cms); if (rc) return rc;                      /* the copy has landed: the maps are whole again, the events can be read */
    for (int i = 0; i < n_ops; ++i) llcms_map(cms, J.ops[i].dst)->broken = false;
    auto span = [&](int a, int b) { return ll_event_ms(G.ev[a], G.ev[b], 0.0); };
    J.ms[0] = span(0, 1); J.ms[1] = span(1, 2) + span(3, 4); J.ms[2] = span(4, 5); J.ms[3] = span(6, 7);
    J.counts[2] = n_out_all;
    return LL_OK;
}

/* the chunks of the counting sort for a record of n points whose first point has the flat index N */
static void mm_close_record(MmRec &R, int rec, long long N, long long n, std::vector<MmChunk> &chunks)
{
    R.first = (int)N; R.pad = 0;
    R.n = (int)n; R.chunk0 = (int)chunks.size(); R.nchunk = (int)((n + MM_CHUNK - 1) / MM_CHUNK);
    for (int k = 0; k < R.nchunk; ++k) chunks.push_back({(int)(N + (long long)k * MM_CHUNK), (int)std::min<long long>(MM_CHUNK, n - (long long)k * MM_CHUNK), rec, 0});
}

extern "C" int ll_cubemaps_merge(ll_cubemaps *cms, const ll_merge_op *ops, int n_ops, long long *added, long long *dropped)
{
    if (!cms) return LL_ERR_ARG;
    if (!ops || n_ops < 1) return llcms_fail(cms, LL_ERR_ARG, "map merge: ops is NULL or n_ops < 1");
    const int S = llcms_size(cms);
    /* ---- every refusal that needs no look at a point: before anything is enqueued */
    std::vector<int> role(S, 0);                                  /* 1: src of some op, 2: dst of one */
    for (int i = 0; i < n_ops; ++i) {
        const ll_merge_op &o = ops[i];
        const std::string who = "map merge: op " + std::to_string(i) + ": ";
        if (o.dst < 0 || o.dst >= S || o.src < 0 || o.src >= S) return llcms_fail(cms, LL_ERR_ARG, who + "dst or src is no map");
        if (o.dst == o.src) return llcms_fail(cms, LL_ERR_ARG, who + "dst and src are the same map");
        for (int k = 0; k < 7; ++k) if (!std::isfinite(o.T_w7[k])) return llcms_fail(cms, LL_ERR_ARG, who + "T is not finite");
        if (role[o.dst] == 2) return llcms_fail(cms, LL_ERR_ARG, who + "map " + std::to_string(o.dst) + " is dst of two ops");
        if (role[o.dst] == 1 || role[o.src] == 2) return llcms_fail(cms, LL_ERR_ARG, who + "a map is dst of one op and src of another");
        role[o.dst] = 2; role[o.src] = 1;
    }
    for (int i = 0; i < n_ops; ++i)
        for (const int q : {ops[i].dst, ops[i].src})
            if (llcms_map(cms, q)->broken) return llcms_fail(cms, LL_ERR_STATE, "map merge: op " + std::to_string(i) + ": map " + std::to_string(q) + " is unusable, an earlier update failed half-way");
    LLMapMerge &G = llcms_merge_state(cms);
    /* ---- the records, the source clouds where they lie, the chunks of the counting sort */
    MmJob J;
    J.what = "map merge: "; J.ms = G.ms; J.counts = G.counts;
    J.recs.resize(2 * n_ops);
    std::vector<MmSeg> segs;
    LLTiler tiles{MM_TILE};
    long long N = 0;
    for (int i = 0; i < n_ops; ++i) {
        const ll_cubemap *src = llcms_map(cms, ops[i].src), *dst = llcms_map(cms, ops[i].dst);
        J.ops.push_back({ops[i].dst, 0, {0, 0, 0}, "map " + std::to_string(ops[i].dst) + " <- map " + std::to_string(ops[i].src)});
        for (int w = 0; w < 2; ++w) {
            MmRec &R = J.recs[2 * i + w];
            for (int k = 0; k < 7; ++k) R.T[k] = ops[i].T_w7[k];
            for (int k = 0; k < 3; ++k) R.cen[k] = dst->cen[k];
            long long n = 0;
            for (int c = 0; c < CM_N; ++c) {
                const int cnt = src->cnt[w][c];
                if (cnt <= 0) continue;
                if (N + n + cnt > (1ll << 30)) return llcms_fail(cms, LL_ERR_CAPACITY, "map merge: more than 2^30 source points in one call");
                segs.push_back({src->pool[w][src->cur[w]] + src->off[w][c], (int)(N + n), cnt, tiles.take(cnt), 2 * i + w});
                n += cnt;
            }
            mm_close_record(R, 2 * i + w, N, n, J.chunks);
            N += n;
        }
    }
    J.N = N;
    const MmSeg *d_segs = nullptr;
    J.stage = [&]() { d_segs = (const MmSeg *)llcms_stage(cms, segs.data(), segs.size() * sizeof(MmSeg)); return d_segs != nullptr; };
    J.assign = [&](const MmRec *d_recs, float4 *d_tp, int *d_keys, int *d_addcnt, hipStream_t st) {
        hipLaunchKernelGGL(k_mm_assign, dim3((unsigned)tiles.next), dim3(256), 0, st, d_segs, (int)segs.size(), d_recs, d_tp, d_keys, d_addcnt);
    };
    return mm_run(cms, J, added, dropped);
}

/* ------------------------------------------------------------------ keyframe insert: one transform per frame through the same stages */
/* v == nullptr: the plain insert.  Otherwise the points that `rule` removes by v's counters are left out and counted in removed */
static int kf_insert(ll_cubemaps *cms, const ll_keyframes *kf, const ll_visibility *v, const ll_visibility_rule *rule, const ll_insert_op *ops, int n_ops,
                     long long *added, long long *dropped, long long *removed)
{
    if (!cms) return LL_ERR_ARG;
    const std::string what = v ? "filtered keyframe insert: " : "keyframe insert: ";
    if (!kf || !ops || n_ops < 1) return llcms_fail(cms, LL_ERR_ARG, what + "kf or ops is NULL, or n_ops < 1");
    if (kf->ctx != llcms_map(cms, 0)->ctx) return llcms_fail(cms, LL_ERR_ARG, what + "the store belongs to another context");
    if (v) {
        if (rule->min_through < 1 || rule->min_through > 256 || rule->max_hit < 0 || rule->max_hit > 255)
            return llcms_fail(cms, LL_ERR_ARG, what + "the rule is outside its ranges (min_through in 1 .. 256, max_hit in 0 .. 255)");
        std::string why;
        const int rc = llvis_check(v, kf, &why);
        if (rc) return llcms_fail(cms, rc, what + why);
    }
    const int S = llcms_size(cms), size = (int)kf->tab.size();
    const ll_keyframe_info *tab = kf->tab.data();
    /* ---- every refusal that needs no look at a point: before anything is enqueued */
    std::vector<char> is_dst(S, 0);
    for (int i = 0; i < n_ops; ++i) {
        const ll_insert_op &o = ops[i];
        const std::string who = what + "op " + std::to_string(i) + ": ";
        if (o.dst < 0 || o.dst >= S) return llcms_fail(cms, LL_ERR_ARG, who + "dst is no map");
        if (is_dst[o.dst]) return llcms_fail(cms, LL_ERR_ARG, who + "map " + std::to_string(o.dst) + " is dst of two ops");
        is_dst[o.dst] = 1;
        if (o.n_frames < 0 || (o.n_frames > 0 && !o.frames)) return llcms_fail(cms, LL_ERR_ARG, who + "n_frames < 0 or frames is NULL");
        if (o.reset != 0 && o.reset != 1) return llcms_fail(cms, LL_ERR_ARG, who + "reset must be 0 or 1");
        if (o.reset)
            for (int k = 0; k < 3; ++k)
                if (o.cen[k] < -(1 << 24) || o.cen[k] > (1 << 24)) return llcms_fail(cms, LL_ERR_ARG, who + "cen[" + std::to_string(k) + "] = " + std::to_string(o.cen[k]) + " is outside the cube array's reach");
        std::string why;
        long long pts;
        if (llkf_check(tab, size, {o.n_frames, o.frames, o.poses_w7, ""}, LLKF_DUP_ALLOWED, nullptr, i, who, &why, &pts)) return llcms_fail(cms, LL_ERR_ARG, why);
    }
    for (int i = 0; i < n_ops; ++i)
        if (llcms_map(cms, ops[i].dst)->broken) return llcms_fail(cms, LL_ERR_STATE, what + "op " + std::to_string(i) + ": map " + std::to_string(ops[i].dst) + " is unusable, an earlier update failed half-way");
    LLMapMerge &G = llcms_merge_state(cms);
    /* ---- the records, the frames' clouds where they lie in the store, each with its frame's pose, the chunks of the counting sort */
    MmJob J;
    J.what = what; J.ms = G.ins_ms; J.counts = G.ins_counts;
    J.recs.resize(2 * n_ops);
    std::vector<KfSeg> segs;
    LLTiler tiles{MM_TILE};
    long long N = 0;
    for (int i = 0; i < n_ops; ++i) {
        const ll_insert_op &o = ops[i];
        const ll_cubemap *dst = llcms_map(cms, o.dst);
        const LLKfList list = {o.n_frames, o.frames, o.poses_w7, ""};
        J.ops.push_back({o.dst, o.reset, {o.cen[0], o.cen[1], o.cen[2]}, "map " + std::to_string(o.dst) + " <- " + std::to_string(o.n_frames) + " keyframes"});
        for (int w = 0; w < 2; ++w) {
            MmRec &R = J.recs[2 * i + w];
            for (int k = 0; k < 7; ++k) R.T[k] = 0.0;             /* not read: the pose is the segment's */
            for (int k = 0; k < 3; ++k) R.cen[k] = o.reset ? o.cen[k] : dst->cen[k];
            long long n = 0;
            for (int f = 0; f < o.n_frames; ++f) {
                const LLKfCloud c = llkf_cloud(tab, kf->cap[0], o.frames[f], w);
                const int cnt = c.cnt;
                if (cnt <= 0) continue;
                if (N + n + cnt > (1ll << 30)) return llcms_fail(cms, LL_ERR_CAPACITY, what + "more than 2^30 source points in one call");
                KfSeg s = {kf->pool + c.off, (int)(N + n), cnt, tiles.take(cnt), 2 * i + w, {}};
                const double *P = llkf_pose(tab, list, f);
                for (int k = 0; k < 7; ++k) s.T[k] = P[k];
                segs.push_back(s);
                n += cnt;
            }
            mm_close_record(R, 2 * i + w, N, n, J.chunks);
            N += n;
        }
    }
    if (!tiles.fits()) return llcms_fail(cms, LL_ERR_CAPACITY, what + "too many tiles for one launch");
    J.N = N;
    const KfSeg *d_segs = nullptr;
    J.stage = [&]() { d_segs = (const KfSeg *)llcms_stage(cms, segs.data(), segs.size() * sizeof(KfSeg)); return d_segs != nullptr; };
    J.filtered = v != nullptr;
    J.assign = [&](const MmRec *d_recs, float4 *d_tp, int *d_keys, int *d_addcnt, hipStream_t st) {
        if (v) {
            const KfFilter F = {kf->pool, v->d_cnt, rule->min_through, rule->max_hit, d_addcnt + (size_t)2 * n_ops * MM_BINS};
            hipLaunchKernelGGL(k_kf_assign<true>, dim3((unsigned)tiles.next), dim3(256), 0, st, d_segs, (int)segs.size(), d_recs, d_tp, d_keys, d_addcnt, F);
        } else {
            const KfFilter F = {nullptr, nullptr, 0, 0, nullptr};
            hipLaunchKernelGGL(k_kf_assign<false>, dim3((unsigned)tiles.next), dim3(256), 0, st, d_segs, (int)segs.size(), d_recs, d_tp, d_keys, d_addcnt, F);
        }
    };
    return mm_run(cms, J, added, dropped, removed);
}

extern "C" int ll_cubemaps_insert_keyframes(ll_cubemaps *cms, const ll_keyframes *kf, const ll_insert_op *ops, int n_ops, long long *added, long long *dropped)
{
    return kf_insert(cms, kf, nullptr, nullptr, ops, n_ops, added, dropped, nullptr);
}

extern "C" int ll_cubemaps_insert_keyframes_filtered(ll_cubemaps *cms, const ll_keyframes *kf, const ll_visibility *v, const ll_visibility_rule *rule,
                                                     const ll_insert_op *ops, int n_ops, long long *added, long long *dropped, long long *removed)
{
    if (!cms) return LL_ERR_ARG;
    if (!v || !rule) return llcms_fail(cms, LL_ERR_ARG, "filtered keyframe insert: the visibility object or the rule is NULL");
    return kf_insert(cms, kf, v, rule, ops, n_ops, added, dropped, removed);
}

extern "C" int ll_cubemaps_insert_timing(const ll_cubemaps *cms, double *ms4, long long *counts3)
{
    if (!cms) return LL_ERR_ARG;
    const LLMapMerge &G = llcms_merge_state(const_cast<ll_cubemaps *>(cms));
    if (ms4) for (int k = 0; k < 4; ++k) ms4[k] = G.ins_ms[k];
    if (counts3) for (int k = 0; k < 3; ++k) counts3[k] = G.ins_counts[k];
    return LL_OK;
}

/* the last ll_cubemaps_merge: ms4 = assign, sort + gather, filter, commit (device events); counts3 = points in, touched cubes, points out */
extern "C" int ll_cubemaps_merge_timing(const ll_cubemaps *cms, double *ms4, long long *counts3)
{
    if (!cms) return LL_ERR_ARG;
    const LLMapMerge &G = llcms_merge_state(const_cast<ll_cubemaps *>(cms));
    if (ms4) for (int k = 0; k < 4; ++k) ms4[k] = G.ms[k];
    if (counts3) for (int k = 0; k < 3; ++k) counts3[k] = G.counts[k];
    return LL_OK;
}
