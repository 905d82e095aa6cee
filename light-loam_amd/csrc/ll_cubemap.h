/*
 * ll_cubemap.h -- what ll_cubemap.hip (one cube map) and ll_cubemaps.hip (S cube maps side by side) share: the cube array's
 * dimensions, the copy descriptor, the state behind an ll_cubemap handle and the host-side bookkeeping of the pair tables.
 */
#pragma once
#include "ll_internal.h"
#include <algorithm>

#define CM_W 21
#define CM_H 21
#define CM_D 11
#define CM_N (CM_W * CM_H * CM_D)     /* 4851 (:53) */
#define CM_MAX_OPS 16384

struct CmOp { int kind, src, cnt, dst, tag; };   /* kind 0: pool[src + i]; kind 1: points[index[src + i]]; tag + i: global id */

/* tile-parallel mapping: the rank that keeps a cube, from the cube's position in the WORLD (array index
 * minus the running centre, which the shifts preserve) so that ownership never changes when the array shifts */
__host__ __device__ __forceinline__ int cm_owner(int wi, int wj, int wk, int world)
{
    const int h = (wi + 3 * wj + 5 * wk) % world;            /* any distance from the origin: the remainder is folded to 0 .. world - 1 */
    return h < 0 ? h + world : h;
}
#define CM_GID_SHIFT 20                  /* global id = position in the valid list << 20 | position in the cube */

struct ll_cubemap {
    ll_ctx *ctx = nullptr;
    ll_map *map = nullptr;
    float leaf[2] = {0.4f, 0.8f};
    int cen[3] = {10, 10, 5};
    int cap_last[2] = {0, 0};
    size_t cap_pool = 0, top[2] = {0, 0};
    float4 *pool[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    int cur[2] = {0, 0};
    std::vector<int> off[2], cnt[2];
    int valid[125]; int n_valid = 0;
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
    std::vector<void *> allocs;
    std::string err;
    bool broken = false;                          /* an update failed half-way: the pair tables no longer describe the pools */
};

#define CM_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) { cm->err = std::string(#call) + ": " + hipGetErrorString(e_); return LL_ERR_HIP; } \
    } while (0)

/* one step of a shift loop (:1598-1778) on the pair tables */
static void cm_shift(ll_cubemap *cm, int axis, int dir)
{
    const int dim[3] = {CM_W, CM_H, CM_D}, stride[3] = {1, CM_W, CM_W * CM_H};
    const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
    for (int w = 0; w < 2; ++w)
        for (int u = 0; u < dim[a1]; ++u) for (int v = 0; v < dim[a2]; ++v) {
            const int base = u * stride[a1] + v * stride[a2];
            std::vector<int> &off = cm->off[w], &cnt = cm->cnt[w];
            if (dir > 0) {
                for (int i = dim[axis] - 1; i >= 1; --i) { off[base + i * stride[axis]] = off[base + (i - 1) * stride[axis]]; cnt[base + i * stride[axis]] = cnt[base + (i - 1) * stride[axis]]; }
                cnt[base] = 0; off[base] = 0;
            } else {
                for (int i = 0; i < dim[axis] - 1; ++i) { off[base + i * stride[axis]] = off[base + (i + 1) * stride[axis]]; cnt[base + i * stride[axis]] = cnt[base + (i + 1) * stride[axis]]; }
                cnt[base + (dim[axis] - 1) * stride[axis]] = 0; off[base + (dim[axis] - 1) * stride[axis]] = 0;
            }
        }
}

/* ll_cubemap.hip: live clouds of type w -> the other pool, back to back; room for `need` more points (compacting when 3/4 full) */
int cm_compact(ll_cubemap *cm, int w);
int cm_reserve(ll_cubemap *cm, int w, size_t need);

/* ll_cubemaps.hip's internals that ll_drives.hip drives (not exported from the library): a frame opens with llcms_begin (the
 * staging arena of the call), may stage tables through it, and maps from the guesses the caller left in llcms_dev_pose [S][7] */
#define LL_HIDDEN __attribute__((visibility("hidden")))
LL_HIDDEN void llcms_begin(ll_cubemaps *cms);
LL_HIDDEN void *llcms_stage(ll_cubemaps *cms, const void *src, size_t bytes);
LL_HIDDEN double *llcms_dev_pose(ll_cubemaps *cms);
LL_HIDDEN long long llcms_syncs(const ll_cubemaps *cms);
LL_HIDDEN const std::string &llcms_err(const ll_cubemaps *cms);
LL_HIDDEN int llcms_process_slots_dev(ll_cubemaps *cms, const int *slots, double *pose_w7, int *ran, const void *extra_dev, void *extra_host,
                                      size_t extra_bytes, ScanHdr *hdr_out);
