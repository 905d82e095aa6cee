/*
 * ll_map_export.hip -- laserMapping's two map publications, laserCloudSurround (laserMapping.cpp:2173-2188, the cubes of
 * laserCloudSurroundInd) and laserCloudMap (:2190-2203, all 4851 cubes), read out of the pools in one gather.
 *
 * The pair tables (off, cnt) live on the host, so the host knows every size before anything is launched: it lists the non-empty
 * clouds as segments (source pointer, destination offset, count) in output order -- per cube the corner cloud, then the surf
 * cloud -- and deals the work in fixed tiles of points.  A full map is thousands of segments between one and several thousand
 * points, most points in a few dozen cubes: a workgroup per segment would leave most workgroups nearly idle and a few with all the
 * work, so a workgroup takes one TILE of one segment and finds the segment by a binary search over the segments' first tiles.
 * The table is uniform per workgroup (scalar loads), points are 16 bytes and every offset is in points (one dwordx4 per lane,
 * consecutive lanes on consecutive points), and all loads of a tile are issued before its first store.  No atomics, no LDS, no
 * workgroup waits on another.
 */
#include "ll_cubemap.h"
#include "ll_tiles.h"
#include <chrono>
#include <cstdlib>

/* one tile = 256 lanes x U points (ll_copy_tile, ll_tiles.h).  The three kernels of this file keep ll_tile_find's loop written out:
 * called as a function the compiler emits its one commutative add (lo + hi) with the operands the other way round, and these
 * kernels' code is kept instruction for instruction */
template <int U>
__global__ __launch_bounds__(256) void k_map_export(const LLExpSeg *seg, int nseg, float4 *dst)
{
    const unsigned t = blockIdx.x;
    int lo = 0, hi = nseg;                                    /* ll_tile_find's loop, written out (see above) */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)__builtin_amdgcn_readfirstlane((int)seg[mid].tile0) <= t) lo = mid; else hi = mid;
    }
    const LLExpSeg s = seg[lo];
    const int first = (int)(t - s.tile0) * (256 * U);
    ll_copy_tile<U, 0>((const ll_gf4 *)(s.src + first), (ll_gf4 *)(dst + s.dst + first), min(256 * U, s.cnt - first), (int)threadIdx.x);
}

/* points per tile: 1024 (four loads in flight per lane) unless LIGHTLOAM_EXPORT_TILE names another of the built sizes (A/B runs:
 * tools/bench_map_export.py, profiles/r09_map_export.json) */
int llx_tile()
{
    if (const char *e = std::getenv("LIGHTLOAM_EXPORT_TILE")) { const int v = std::atoi(e); if (v == 256 || v == 512 || v == 1024 || v == 2048) return v; }
    return 1024;
}

/* the clouds of `cm` that `which` selects, in output order from point dst0 on, numbered by T.  Returns the number of points;
 * T == nullptr: sizes only */
long long llx_segments(const ll_cubemap *cm, int which, long long dst0, LLTiler *T, std::vector<LLExpSeg> *segs)
{
    long long at = dst0;
    const int n = which == LL_MAP_ALL ? CM_N : which == LL_MAP_SURROUND ? cm->n_valid : 0;
    for (int v = 0; v < n; ++v) {
        const int c = which == LL_MAP_ALL ? v : cm->valid[v];
        for (int w = 0; w < 2; ++w) {
            const int cnt = cm->cnt[w][c];
            if (cnt <= 0) continue;
            if (T) segs->push_back({cm->pool[w][cm->cur[w]] + cm->off[w][c], at, cnt, T->take(cnt)});
            at += cnt;
        }
    }
    return at - dst0;
}

/* segs -> page-locked memory -> device, for the object that has no per-call arena */
const void *llx_stage_bytes(LLMapExport &X, const void *data, size_t bytes, hipStream_t st, std::string &err)
{
    if (bytes > X.cap_tab) {
        const size_t cap = std::max<size_t>(std::max<size_t>(2 * X.cap_tab, bytes), (size_t)1 << 16);
        if (X.h_tab) (void)hipHostFree(X.h_tab);
        if (X.d_tab) (void)hipFree(X.d_tab);
        X.h_tab = nullptr; X.d_tab = nullptr; X.cap_tab = 0;
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, cap, hipHostMallocDefault) != hipSuccess || hipMalloc(&d, cap) != hipSuccess) {
            if (h) (void)hipHostFree(h);
            (void)hipGetLastError();
            err = "map export: no memory for the segment table (" + std::to_string(cap) + " bytes)"; return nullptr;
        }
        X.h_tab = (unsigned char *)h; X.d_tab = (unsigned char *)d; X.cap_tab = cap;
    }
    std::memcpy(X.h_tab, data, bytes);
    if (hipMemcpyAsync(X.d_tab, X.h_tab, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { err = "map export: upload failed"; return nullptr; }
    return X.d_tab;
}

const LLExpSeg *llx_stage(LLMapExport &X, const std::vector<LLExpSeg> &segs, hipStream_t st, std::string &err)
{
    return (const LLExpSeg *)llx_stage_bytes(X, segs.data(), segs.size() * sizeof(LLExpSeg), st, err);
}

bool llx_is_device(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   /* plain host memory the runtime has never seen */
    return a.type == hipMemoryTypeDevice;
}

/* ONE gather of `total` points over the staged table, one copy to `out`, ONE synchronisation.  limit: the most points the
 * staging buffer may ever need (the pools' live points cannot exceed it) */
int llx_gather(LLMapExport &X, ll_ctx *ctx, const LLExpSeg *d_segs, size_t nseg, unsigned long long ntiles, long long total, size_t limit,
               int tile_points, ll_point *out, std::string &err)
{
    hipStream_t st = ctx->stream;
    if (!X.have_ev) {
        for (int k = 0; k < 3; ++k) if (hipEventCreate(&X.ev[k]) != hipSuccess) { for (int j = 0; j < k; ++j) (void)hipEventDestroy(X.ev[j]); err = "map export: hipEventCreate failed"; return LL_ERR_HIP; }
        X.have_ev = true;
    }
    float4 *dst = (float4 *)out;
    const bool direct = total > 0 && llx_is_device(out);
    if (total > 0 && !direct) {
        if ((size_t)total > X.cap_dst) {
            const size_t cap = std::min(std::max<size_t>((size_t)total, 2 * X.cap_dst), std::max<size_t>(limit, (size_t)total));
            if (X.d_dst) (void)hipFree(X.d_dst);
            X.d_dst = nullptr; X.cap_dst = 0;
            void *p = nullptr;
            if (hipMalloc(&p, cap * sizeof(float4)) != hipSuccess) {
                (void)hipGetLastError();
                err = "map export: hipMalloc failed for the staging buffer (" + std::to_string(cap * sizeof(float4)) + " bytes)"; return LL_ERR_HIP;
            }
            X.d_dst = (float4 *)p; X.cap_dst = cap;
        }
        dst = X.d_dst;
    }
    hipError_t e = hipEventRecord(X.ev[0], st);
    if (e == hipSuccess && total > 0) {
        const dim3 grid((unsigned)ntiles), block(256);
        switch (tile_points) {
        case 256: hipLaunchKernelGGL(k_map_export<1>, grid, block, 0, st, d_segs, (int)nseg, dst); break;
        case 512: hipLaunchKernelGGL(k_map_export<2>, grid, block, 0, st, d_segs, (int)nseg, dst); break;
        case 2048: hipLaunchKernelGGL(k_map_export<8>, grid, block, 0, st, d_segs, (int)nseg, dst); break;
        default: hipLaunchKernelGGL(k_map_export<4>, grid, block, 0, st, d_segs, (int)nseg, dst); break;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(X.ev[1], st);
    if (e == hipSuccess && total > 0 && !direct) e = hipMemcpyAsync(out, dst, (size_t)total * sizeof(float4), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(X.ev[2], st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { err = std::string("map export: ") + hipGetErrorString(e); return LL_ERR_HIP; }
    X.ms[1] = ll_event_ms(X.ev[0], X.ev[1], -1.0);
    X.ms[2] = ll_event_ms(X.ev[1], X.ev[2], -1.0);
    X.points = total; X.segments = (long long)nseg; X.tiles = (long long)ntiles;
    return LL_OK;
}

void llx_free(LLMapExport &X)
{
    if (X.d_dst) (void)hipFree(X.d_dst);
    if (X.d_tab) (void)hipFree(X.d_tab);
    if (X.h_tab) (void)hipHostFree(X.h_tab);
    if (X.have_ev) for (int k = 0; k < 3; ++k) (void)hipEventDestroy(X.ev[k]);
    X = LLMapExport();
}

void llx_timing(const LLMapExport &X, double *ms3, long long *counts3)
{
    if (ms3) for (int k = 0; k < 3; ++k) ms3[k] = X.ms[k];
    if (counts3) { counts3[0] = X.points; counts3[1] = X.segments; counts3[2] = X.tiles; }
}

/* ------------------------------------------------------------------ map import: the export's inverse
 * The input is the byte layout an LL_MAP_ALL export writes (cubes 0 .. 4850, per cube the corner cloud, then the surf cloud); the
 * host knows every size from `counts`, lists the non-empty clouds as segments in INPUT order and deals the work in the same
 * fixed tiles: a workgroup takes one tile of one segment, found by the same binary search over the segments' first tiles
 * (scalar loads), and copies it with ll_copy_tile -- one dwordx4 load and one dwordx4 store per lane per point, every load of
 * the tile before its first store.  The corner and surf clouds of a cube are neighbours in the input and go to two different
 * pools: the de-interleave is in the segments' destinations.  No atomics, no LDS, no workgroup waits on another. */
template <int U>
__global__ __launch_bounds__(256) void k_map_import(const LLImpSeg *seg, int nseg, const float4 *src)
{
    const unsigned t = blockIdx.x;
    int lo = 0, hi = nseg;                                    /* ll_tile_find's loop, written out (see above) */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)__builtin_amdgcn_readfirstlane((int)seg[mid].tile0) <= t) lo = mid; else hi = mid;
    }
    const LLImpSeg s = seg[lo];
    const int first = (int)(t - s.tile0) * (256 * U);
    ll_copy_tile<U, 0>((const ll_gf4 *)(src + s.src + first), (ll_gf4 *)(s.dst + first), min(256 * U, s.cnt - first), (int)threadIdx.x);
}

/* the checkpoint pack launch: workgroups [0, ntiles) are k_map_export's tiles; behind them R + 1 workgroups per record -- ring r
 * of the record's ring-strided less-flat cloud closed up through lf_pre (k_lflat_flatten's order), and the lane's 22 doubles
 * and frame counter (the pose arrays are 8-byte aligned: they cannot go through the 16-byte tiles) */
template <int U>
__global__ __launch_bounds__(256) void k_ckpt_pack(const LLExpSeg *seg, int nseg, unsigned ntiles, const LLCkRec *rec, int R, float4 *dst)
{
    unsigned t = blockIdx.x;
    const int tid = (int)threadIdx.x;
    if (t < ntiles) {
        int lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((unsigned)__builtin_amdgcn_readfirstlane((int)seg[mid].tile0) <= t) lo = mid; else hi = mid;
        }
        const LLExpSeg s = seg[lo];
        const int first = (int)(t - s.tile0) * (256 * U);
        ll_copy_tile<U, 0>((const ll_gf4 *)(s.src + first), (ll_gf4 *)(dst + s.dst + first), min(256 * U, s.cnt - first), tid);
        return;
    }
    t -= ntiles;
    const int r = (int)(t / (unsigned)(R + 1)), ring = (int)(t - (unsigned)r * (unsigned)(R + 1));
    const LLCkRec c = rec[r];
    if (ring < R) {
        if (!c.lflat) return;
        const int o = c.lf_pre[ring], n = c.lf_pre[ring + 1] - o;
        /* never beyond the row, nor beyond what the host sized the record for: a table that disagrees with the header the host
         * read is reported (the save fails), not packed short */
        if (o < 0 || n < 0 || n > c.ring_cap || o + n > c.n_lflat || (ring == R - 1 && o + n != c.n_lflat)) { if (tid == 0) *c.bad = 1; return; }
        for (int i = tid; i < n; i += 256) dst[c.dst_lflat + o + i] = c.lflat[(size_t)ring * c.ring_cap + i];
    } else {
        double *out = (double *)(dst + c.dst_state);
        if (tid < 7) { out[tid] = c.pose[tid]; out[7 + tid] = c.odom[tid]; out[14 + tid] = c.m2o[tid]; }
        if (tid == 0) { int *f = (int *)(out + 21); f[0] = c.fidx[0]; f[1] = 0; }
    }
}

int llx_pack(ll_ctx *ctx, const LLExpSeg *d_segs, size_t nseg, unsigned long long ntiles, const LLCkRec *d_rec, int nrec, int R, int tile_points, float4 *dst, std::string &err)
{
    const unsigned long long nb = ntiles + (unsigned long long)nrec * (unsigned)(R + 1);
    if (nb == 0) return LL_OK;
    if (!ll_grid_fits(nb)) { err = "checkpoint: too many tiles for one launch"; return LL_ERR_CAPACITY; }
    const dim3 grid((unsigned)nb), block(256);
    hipStream_t st = ctx->stream;
    switch (tile_points) {
    case 256: hipLaunchKernelGGL(k_ckpt_pack<1>, grid, block, 0, st, d_segs, (int)nseg, (unsigned)ntiles, d_rec, R, dst); break;
    case 512: hipLaunchKernelGGL(k_ckpt_pack<2>, grid, block, 0, st, d_segs, (int)nseg, (unsigned)ntiles, d_rec, R, dst); break;
    case 2048: hipLaunchKernelGGL(k_ckpt_pack<8>, grid, block, 0, st, d_segs, (int)nseg, (unsigned)ntiles, d_rec, R, dst); break;
    default: hipLaunchKernelGGL(k_ckpt_pack<4>, grid, block, 0, st, d_segs, (int)nseg, (unsigned)ntiles, d_rec, R, dst); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("checkpoint pack: ") + hipGetErrorString(e); return LL_ERR_HIP; }
    return LL_OK;
}

int llx_import_check(const ll_cubemap *cm, const int *cen3, const int *counts, const int *valid, int n_valid, long long n_points, std::string &err)
{
    /* the centre is the array index of the world's origin cube: it leaves [0, 21) as soon as the map has shifted far enough (a drive
     * of a few hundred metres), so it is bounded only where the cube arithmetic (:1584-1586, k_cm_assign) would overflow */
    for (int k = 0; k < 3; ++k) if (cen3[k] < -(1 << 24) || cen3[k] > (1 << 24)) { err = "cen[" + std::to_string(k) + "] = " + std::to_string(cen3[k]) + " is outside the cube array's reach"; return LL_ERR_ARG; }
    if (n_valid < 0 || n_valid > 125) { err = "n_valid = " + std::to_string(n_valid) + " is not in 0..125"; return LL_ERR_ARG; }
    std::vector<char> seen(CM_N, 0);
    for (int v = 0; v < n_valid; ++v) {
        if (valid[v] < 0 || valid[v] >= CM_N || seen[valid[v]]) { err = "valid[" + std::to_string(v) + "] = " + std::to_string(valid[v]) + " is out of range or listed twice"; return LL_ERR_ARG; }
        seen[valid[v]] = 1;
    }
    long long tot[2] = {0, 0};
    for (int w = 0; w < 2; ++w)
        for (int c = 0; c < CM_N; ++c) {
            const int n = counts[(size_t)w * CM_N + c];
            if (n < 0) { err = "counts[" + std::to_string(w) + "][" + std::to_string(c) + "] is negative"; return LL_ERR_ARG; }
            if (n > 0 && cm->world > 1) {
                const int ci = c % CM_W, cj = (c / CM_W) % CM_H, ck = c / (CM_W * CM_H);
                if (cm_owner(ci - cen3[0], cj - cen3[1], ck - cen3[2], cm->world) != cm->rank) { err = "cube " + std::to_string(c) + " belongs to another tile shard"; return LL_ERR_ARG; }
                if (n >= (1 << CM_GID_SHIFT)) { err = "cube " + std::to_string(c) + " holds more points than a tile shard can number"; return LL_ERR_CAPACITY; }
            }
            tot[w] += n;
        }
    if (n_points >= 0 && tot[0] + tot[1] != n_points) { err = "counts add up to " + std::to_string(tot[0] + tot[1]) + " points, the input holds " + std::to_string(n_points); return LL_ERR_ARG; }
    for (int w = 0; w < 2; ++w)
        if ((unsigned long long)tot[w] > (unsigned long long)cm->cap_pool) { err = std::to_string(tot[w]) + (w ? " surf" : " corner") + " points, pool_points is " + std::to_string(cm->cap_pool); return LL_ERR_CAPACITY; }
    return LL_OK;
}

void llx_import_segments(const ll_cubemap *cm, const int *counts, long long src0, LLTiler &T, std::vector<LLImpSeg> *segs)
{
    long long at = src0;
    size_t top[2] = {0, 0};
    for (int c = 0; c < CM_N; ++c)
        for (int w = 0; w < 2; ++w) {
            const int cnt = counts[(size_t)w * CM_N + c];
            if (cnt <= 0) continue;
            segs->push_back({cm->pool[w][0] + top[w], at, cnt, T.take(cnt)});
            at += cnt; top[w] += (size_t)cnt;
        }
}

void llx_import_commit(ll_cubemap *cm, const int *cen3, const int *counts, const int *valid, int n_valid)
{
    for (int k = 0; k < 3; ++k) cm->cen[k] = cen3[k];
    for (int w = 0; w < 2; ++w) {
        size_t top = 0;
        for (int c = 0; c < CM_N; ++c) {
            const int cnt = counts[(size_t)w * CM_N + c];
            cm->off[w][c] = cnt > 0 ? (int)top : 0; cm->cnt[w][c] = cnt; top += (size_t)cnt;
        }
        cm->top[w] = top; cm->cur[w] = 0;
        cm->map->M.n_map[w] = 0; cm->map->M.n_stk[w] = 0;
    }
    cm->n_valid = n_valid;
    for (int v = 0; v < n_valid; ++v) cm->valid[v] = valid[v];
    cm->broken = false; cm->has_frame = false;
}

float4 *llx_reserve(LLMapExport &X, size_t n, std::string &err)
{
    if (n > X.cap_dst) {
        const size_t cap = std::max<size_t>(n, 2 * X.cap_dst);
        void *p = nullptr;
        if (hipMalloc(&p, cap * sizeof(float4)) != hipSuccess) {         /* the old buffer is kept: the object stays as it was */
            (void)hipGetLastError();
            err = "hipMalloc failed for the staging buffer (" + std::to_string(cap * sizeof(float4)) + " bytes)"; return nullptr;
        }
        if (X.d_dst) (void)hipFree(X.d_dst);                              /* hipFree waits for the work that may still read it */
        X.d_dst = (float4 *)p; X.cap_dst = cap;
    }
    return X.d_dst;
}

int llx_scatter(ll_ctx *ctx, const LLImpSeg *d_segs, size_t nseg, unsigned long long ntiles, float4 *src, const void *up, size_t n_up, int tile_points, std::string &err)
{
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    if (up && n_up > 0) e = hipMemcpyAsync(src, up, n_up * sizeof(float4), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && ntiles > 0) {
        const dim3 grid((unsigned)ntiles), block(256);
        switch (tile_points) {
        case 256: hipLaunchKernelGGL(k_map_import<1>, grid, block, 0, st, d_segs, (int)nseg, (const float4 *)src); break;
        case 512: hipLaunchKernelGGL(k_map_import<2>, grid, block, 0, st, d_segs, (int)nseg, (const float4 *)src); break;
        case 2048: hipLaunchKernelGGL(k_map_import<8>, grid, block, 0, st, d_segs, (int)nseg, (const float4 *)src); break;
        default: hipLaunchKernelGGL(k_map_import<4>, grid, block, 0, st, d_segs, (int)nseg, (const float4 *)src); break;
        }
        e = hipGetLastError();
    }
    if (e != hipSuccess) { err = std::string("map import: ") + hipGetErrorString(e); return LL_ERR_HIP; }
    return LL_OK;
}

/* ------------------------------------------------------------------ the single cube map (the ROS node's map) */
extern "C" int ll_cubemap_export(ll_cubemap *cm, int which, ll_point *out, long long cap, long long *n)
{
    if (!cm) return LL_ERR_ARG;
    if (which < LL_MAP_NONE || which > LL_MAP_ALL || cap < 0) { cm->err = "map export: bad arguments"; return LL_ERR_ARG; }
    if (which != LL_MAP_NONE && cm->broken) { cm->err = "the cube map is unusable: an earlier ll_cubemap_update failed half-way"; return LL_ERR_STATE; }
    const auto t0 = std::chrono::steady_clock::now();
    LLTiler T{llx_tile()};
    std::vector<LLExpSeg> segs;
    const long long total = llx_segments(cm, which, 0, &T, &segs);
    if (n) *n = total;
    if (total > 0 && !out) { cm->err = "map export: out is NULL"; return LL_ERR_ARG; }
    if (total > cap) { cm->err = "map export: " + std::to_string(total) + " points, room for " + std::to_string(cap); return LL_ERR_CAPACITY; }
    if (!T.fits()) { cm->err = "map export: too many tiles for one launch"; return LL_ERR_CAPACITY; }
    CM_HIP(hipSetDevice(cm->ctx->device));
    const LLExpSeg *d_segs = nullptr;
    if (total > 0) { d_segs = llx_stage(cm->X, segs, cm->ctx->stream, cm->err); if (!d_segs) return LL_ERR_HIP; }
    cm->X.ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return llx_gather(cm->X, cm->ctx, d_segs, segs.size(), T.next, total, 2 * cm->cap_pool, T.per, out, cm->err);
}

extern "C" int ll_cubemap_layout(ll_cubemap *cm, int *cen3, int *counts, int *valid, int *n_valid)
{
    if (!cm) return LL_ERR_ARG;
    if (cen3) for (int k = 0; k < 3; ++k) cen3[k] = cm->cen[k];
    if (counts) for (int w = 0; w < 2; ++w) std::memcpy(counts + (size_t)w * CM_N, cm->cnt[w].data(), CM_N * sizeof(int));
    if (valid) for (int v = 0; v < cm->n_valid; ++v) valid[v] = cm->valid[v];
    if (n_valid) *n_valid = cm->n_valid;
    return LL_OK;
}

extern "C" int ll_cubemap_import(ll_cubemap *cm, const ll_point *points, long long n, const int *cen3, const int *counts, const int *valid, int n_valid)
{
    if (!cm) return LL_ERR_ARG;
    if (n < 0 || (n > 0 && !points) || !cen3 || !counts || (n_valid > 0 && !valid)) { cm->err = "map import: bad arguments"; return LL_ERR_ARG; }
    std::string why;
    int rc = llx_import_check(cm, cen3, counts, valid, n_valid, n, why);
    if (rc) { cm->err = "map import: " + why; return rc; }
    LLTiler T{llx_tile()};
    std::vector<LLImpSeg> segs;
    llx_import_segments(cm, counts, 0, T, &segs);
    if (!T.fits()) { cm->err = "map import: too many tiles for one launch"; return LL_ERR_CAPACITY; }
    CM_HIP(hipSetDevice(cm->ctx->device));
    const bool direct = n > 0 && llx_is_device(points);
    float4 *src = direct ? (float4 *)points : nullptr;
    if (n > 0 && !direct) { src = llx_reserve(cm->X, (size_t)n, why); if (!src) { cm->err = "map import: " + why; return LL_ERR_HIP; } }
    const LLImpSeg *d_segs = nullptr;
    if (n > 0) {
        d_segs = (const LLImpSeg *)llx_stage_bytes(cm->X, segs.data(), segs.size() * sizeof(LLImpSeg), cm->ctx->stream, cm->err);
        if (!d_segs) return LL_ERR_HIP;
    }
    cm->broken = true;                                        /* until the scatter has landed */
    rc = llx_scatter(cm->ctx, d_segs, segs.size(), T.next, src, direct ? nullptr : points, (size_t)n, T.per, cm->err);
    if (rc) return rc;
    CM_HIP(hipStreamSynchronize(cm->ctx->stream));
    llx_import_commit(cm, cen3, counts, valid, n_valid);
    return LL_OK;
}
