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
#include <chrono>
#include <cstdlib>

/* point K * 256 + tid of a tile of n >= 1 points: the loads of all U points are issued before the first store (a clamped index
 * instead of a branch between them; the recursion keeps the U values in registers) */
typedef float llx_f4 __attribute__((ext_vector_type(4)));
typedef llx_f4 __attribute__((address_space(1))) llx_gf4;    /* the pointers come out of a table: said to be global, not flat */
template <int U, int K>
__device__ __forceinline__ void llx_copy_tile(const llx_gf4 *src, llx_gf4 *out, int n, int tid)
{
    const int i = K * 256 + tid;
    const llx_f4 v = src[min(i, n - 1)];
    if constexpr (K + 1 < U) llx_copy_tile<U, K + 1>(src, out, n, tid);
    if (i < n) out[i] = v;
}

/* one tile = 256 lanes x U points */
template <int U>
__global__ __launch_bounds__(256) void k_map_export(const LLExpSeg *seg, int nseg, float4 *dst)
{
    const unsigned t = blockIdx.x;
    int lo = 0, hi = nseg;                                    /* the last segment whose first tile is <= t */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)__builtin_amdgcn_readfirstlane((int)seg[mid].tile0) <= t) lo = mid; else hi = mid;
    }
    const LLExpSeg s = seg[lo];
    const int first = (int)(t - s.tile0) * (256 * U);
    llx_copy_tile<U, 0>((const llx_gf4 *)(s.src + first), (llx_gf4 *)(dst + s.dst + first), min(256 * U, s.cnt - first), (int)threadIdx.x);
}

/* points per tile: 1024 (four loads in flight per lane) unless LIGHTLOAM_EXPORT_TILE names another of the built sizes (A/B runs:
 * tools/bench_map_export.py, profiles/r09_map_export.json) */
int llx_tile()
{
    if (const char *e = std::getenv("LIGHTLOAM_EXPORT_TILE")) { const int v = std::atoi(e); if (v == 256 || v == 512 || v == 1024 || v == 2048) return v; }
    return 1024;
}

/* the clouds of `cm` that `which` selects, in output order from point dst0 on; *tile: the running number of tiles.  Returns the
 * number of points; segs == nullptr: sizes only */
long long llx_segments(const ll_cubemap *cm, int which, long long dst0, int tile_points, unsigned long long *tile, std::vector<LLExpSeg> *segs)
{
    long long at = dst0;
    const int n = which == LL_MAP_ALL ? CM_N : which == LL_MAP_SURROUND ? cm->n_valid : 0;
    for (int v = 0; v < n; ++v) {
        const int c = which == LL_MAP_ALL ? v : cm->valid[v];
        for (int w = 0; w < 2; ++w) {
            const int cnt = cm->cnt[w][c];
            if (cnt <= 0) continue;
            if (segs) {
                segs->push_back({cm->pool[w][cm->cur[w]] + cm->off[w][c], at, cnt, (unsigned)*tile});
                *tile += (unsigned long long)((cnt + tile_points - 1) / tile_points);
            }
            at += cnt;
        }
    }
    return at - dst0;
}

/* segs -> page-locked memory -> device, for the object that has no per-call arena */
const LLExpSeg *llx_stage(LLMapExport &X, const std::vector<LLExpSeg> &segs, hipStream_t st, std::string &err)
{
    const size_t bytes = segs.size() * sizeof(LLExpSeg);
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
    std::memcpy(X.h_tab, segs.data(), bytes);
    if (hipMemcpyAsync(X.d_tab, X.h_tab, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { err = "map export: upload failed"; return nullptr; }
    return (const LLExpSeg *)X.d_tab;
}

static bool llx_is_device(const void *p)
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
    float ms = 0.0f;
    X.ms[1] = hipEventElapsedTime(&ms, X.ev[0], X.ev[1]) == hipSuccess ? (double)ms : -1.0;
    X.ms[2] = hipEventElapsedTime(&ms, X.ev[1], X.ev[2]) == hipSuccess ? (double)ms : -1.0;
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

/* ------------------------------------------------------------------ the single cube map (the ROS node's map) */
extern "C" int ll_cubemap_export(ll_cubemap *cm, int which, ll_point *out, long long cap, long long *n)
{
    if (!cm) return LL_ERR_ARG;
    if (which < LL_MAP_NONE || which > LL_MAP_ALL || cap < 0) { cm->err = "map export: bad arguments"; return LL_ERR_ARG; }
    if (which != LL_MAP_NONE && cm->broken) { cm->err = "the cube map is unusable: an earlier ll_cubemap_update failed half-way"; return LL_ERR_STATE; }
    const auto t0 = std::chrono::steady_clock::now();
    const int tile_points = llx_tile();
    std::vector<LLExpSeg> segs;
    unsigned long long ntiles = 0;
    const long long total = llx_segments(cm, which, 0, tile_points, &ntiles, &segs);
    if (n) *n = total;
    if (total > 0 && !out) { cm->err = "map export: out is NULL"; return LL_ERR_ARG; }
    if (total > cap) { cm->err = "map export: " + std::to_string(total) + " points, room for " + std::to_string(cap); return LL_ERR_CAPACITY; }
    if (ntiles > 0x7fffffffull) { cm->err = "map export: too many tiles for one launch"; return LL_ERR_CAPACITY; }
    CM_HIP(hipSetDevice(cm->ctx->device));
    const LLExpSeg *d_segs = nullptr;
    if (total > 0) { d_segs = llx_stage(cm->X, segs, cm->ctx->stream, cm->err); if (!d_segs) return LL_ERR_HIP; }
    cm->X.ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return llx_gather(cm->X, cm->ctx, d_segs, segs.size(), ntiles, total, 2 * cm->cap_pool, tile_points, out, cm->err);
}
