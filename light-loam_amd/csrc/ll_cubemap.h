/*
 * ll_cubemap.h -- what ll_cubemap.hip (one cube map) and ll_cubemaps.hip (S cube maps side by side) share: the device-side cube
 * arithmetic, the copy descriptor and the state behind an ll_cubemap handle.  The cube array's dimensions and the host-side
 * bookkeeping of the pair tables are ll_cubemap_tables.h; a map embeds its export state, so ll_map_export.h comes with it.  What
 * the many-maps object adds (merge and align workspaces, its internal interface) and the keyframe store with its readers have
 * headers of their own, which include this one or ll_map_export.h -- never the other way round.
 */
#pragma once
#include "ll_internal.h"
#include "ll_map_search.h"
#include "ll_cubemap_tables.h"
#include "ll_map_export.h"

#define CM_MAX_OPS 16384

struct CmOp { int kind, src, cnt, dst, tag; };   /* kind 0: pool[src + i]; kind 1: points[index[src + i]]; tag + i: global id */

/* tile-parallel mapping: the rank that keeps a cube, from the cube's position in the WORLD (array index
 * minus the running centre, which the shifts preserve) so that ownership never changes when the array shifts */
__host__ __device__ __forceinline__ int cm_owner(int wi, int wj, int wk, int world)
{
    const int h = (wi + 3 * wj + 5 * wk) % world;            /* any distance from the origin: the remainder is folded to 0 .. world - 1 */
    return h < 0 ? h + world : h;
}

/* the cube a world point falls into (:2108-2125) in the array centred at cen: its three indices, and the cube index or -1 outside */
__device__ __forceinline__ int cm_cube_of(float sx, float sy, float sz, const int cen[3], int *ci, int *cj, int *ck)
{
    int i = (int)(((double)sx + 25.0) / 50.0) + cen[0], j = (int)(((double)sy + 25.0) / 50.0) + cen[1], k = (int)(((double)sz + 25.0) / 50.0) + cen[2];
    if ((double)sx + 25.0 < 0) i--;
    if ((double)sy + 25.0 < 0) j--;
    if ((double)sz + 25.0 < 0) k--;
    *ci = i; *cj = j; *ck = k;
    return (i >= 0 && i < CM_W && j >= 0 && j < CM_H && k >= 0 && k < CM_D) ? i + CM_W * j + CM_W * CM_H * k : -1;
}

/* addcnt[cube] += the lanes of this wave with that cube (cube < 0: not counted).  The points of a scan fall into a handful of
 * cubes: one add per wave and cube, not one per point on the same address.  Every lane of the wave has to call it */
__device__ __forceinline__ void cm_wave_count(int cube, int *addcnt)
{
    unsigned long long todo = __ballot(cube >= 0);
    while (todo) {
        const int c0 = __shfl(cube, __ffsll((long long)todo) - 1);
        const unsigned long long same = __ballot(cube == c0);
        if ((threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(&addcnt[c0], __popcll(same));
        todo &= ~same;
    }
}

/* stack point i of one cube map's update: pointAssociateToMap (:125-134) into tp, its cube as the sort key (CM_N: outside the
 * array, or -- world > 1 -- another rank's cube: not kept here), vals = i, and the per-cube counts.  Called by whole waves */
__device__ __forceinline__ void cm_assign_one(const float4 *stk, int n, const double *pose, const int cen[3], int rank, int world,
                                              float4 *tp, unsigned long long *keys, int *vals, int *addcnt, int i)
{
    int cube = -1;                                            /* -1: no point / not counted */
    if (i < n) {
        const float4 po = stk[i];
        float sx, sy, sz;
        ll_map_to_world(pose, po, sx, sy, sz);
        tp[i] = make_float4(sx, sy, sz, po.w);
        int ci, cj, ck;
        cube = cm_cube_of(sx, sy, sz, cen, &ci, &cj, &ck);
        if (cube >= 0 && world != 1 && cm_owner(ci - cen[0], cj - cen[1], ck - cen[2], world) != rank) cube = -1;
        keys[i] = (unsigned long long)(cube >= 0 ? cube : CM_N);
        vals[i] = i;
    }
    cm_wave_count(cube, addcnt);
}
#define CM_GID_SHIFT 20                  /* global id = position in the valid list << 20 | position in the cube */

struct ll_cubemap : CmTables {                   /* the pair tables (ll_cubemap_tables.h) and the device memory they describe */
    ll_ctx *ctx = nullptr;
    ll_map *map = nullptr;
    float leaf[2] = {0.4f, 0.8f};
    int cap_last[2] = {0, 0};
    float4 *pool[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    int rank = 0, world = 1;                      /* tile shard: this map keeps the cubes with cm_owner() == rank */
    float4 *d_last = nullptr;
    /* ll_cubemap_update runs both cloud types through every stage before it synchronises: one set of buffers per type */
    float4 *d_tp[2] = {nullptr, nullptr}, *d_work[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};
    int cap_work = 0;
    CmOp *d_ops = nullptr;
    int *d_addcnt = nullptr, *d_nout = nullptr;   /* [2][CM_N + 1]; [4]: stack sizes of prepare, filtered sizes of update */
    unsigned long long *d_keys[2] = {nullptr, nullptr}; int *d_vals[2] = {nullptr, nullptr};
    void *vox_mem = nullptr; LLVoxWork W;         /* prepare's filters and update's corner filter */
    void *vox_mem2 = nullptr; LLVoxWork W2;       /* update's surface filter */
    void *sort_mem = nullptr; LLVoxWork WS;       /* scratch of the by-cube sort (same layout, stack-sized) */
    LLMapExport X;                                /* ll_cubemap_export's buffers (not used by the maps inside an ll_cubemaps) */
    std::vector<void *> allocs;
    std::string err;
    bool broken = false;                          /* an update failed half-way: the pair tables no longer describe the pools */
    bool has_frame = false;                       /* a frame has run since create / reset / import: the stack clouds are one frame's (the keyframe store) */
};

#define CM_HIP(call) LL_HIP_CHECK(ll_fail, cm, "", call, #call)

/* ll_cubemap.hip: a compaction's copies (cm_commit's moves) of type w, out of the pool that was current into the one that is */
void cm_run_moves(ll_cubemap *cm, int w, const std::vector<CmPiece> &moves);
