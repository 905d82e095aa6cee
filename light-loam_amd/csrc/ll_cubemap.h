/*
 * ll_cubemap.h -- what ll_cubemap.hip (one cube map) and ll_cubemaps.hip (S cube maps side by side) share: the device-side cube
 * arithmetic, the copy descriptor and the state behind an ll_cubemap handle.  The cube array's dimensions and the host-side
 * bookkeeping of the pair tables are ll_cubemap_tables.h.
 */
#pragma once
#include "ll_internal.h"
#include "ll_map_search.h"
#include "ll_cubemap_tables.h"

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
/* the last segment whose first tile is <= t: the tables of the tiled kernels (map merge, keyframe insert, visibility) */
template <typename S>
__device__ __forceinline__ int mm_find(const S *seg, int nseg, unsigned t)
{
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)__builtin_amdgcn_readfirstlane((int)seg[mid].tile0) <= t) lo = mid; else hi = mid;
    }
    return lo;
}
#define CM_GID_SHIFT 20                  /* global id = position in the valid list << 20 | position in the cube */

/* map export (ll_map_export.hip): one non-empty cloud of the output.  dst: its first point in the output; tile0: the tiles of
 * the segments before it */
struct LLExpSeg { const float4 *src; long long dst; int cnt; unsigned tile0; };
/* what an exporting object keeps between calls: the device staging buffer of the gathered cloud (grown to the need), the
 * page-locked / device pair the single map's table goes through, the events around the gather and the copy of the last call */
struct LLMapExport {
    float4 *d_dst = nullptr; size_t cap_dst = 0;
    unsigned char *h_tab = nullptr, *d_tab = nullptr; size_t cap_tab = 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr}; bool have_ev = false;
    double ms[3] = {0.0, 0.0, 0.0};               /* the last export: table build (host clock), gather, copy (events) */
    long long points = 0, segments = 0, tiles = 0;
};

/* map merge (ll_map_merge.hip): what a merging object keeps between calls -- two device buffers grown to the need (0: the by-cube
 * order of the source points, 1: the filters' input, output and workspace), the events around the stages, the last call's figures */
#define LL_MM_EVENTS 8
struct LLMapMerge {
    unsigned char *d_mem[2] = {nullptr, nullptr}; size_t cap_mem[2] = {0, 0};
    hipEvent_t ev[LL_MM_EVENTS] = {}; bool have_ev = false;
    double ms[4] = {0.0, 0.0, 0.0, 0.0};          /* the last merge: assign, sort + gather, filter, commit (events) */
    long long counts[3] = {0, 0, 0};              /* points in, touched cubes, points out */
    double ins_ms[4] = {0.0, 0.0, 0.0, 0.0};      /* the same of the last ll_cubemaps_insert_keyframes, which runs in the same workspace */
    long long ins_counts[3] = {0, 0, 0};
};

/* keyframes (ll_keyframes.hip): the stack clouds of mapped frames, type w in region w of ONE allocation (region 1 begins at
 * cap[0]), a frame's cloud at tab[id].offset[w] of its region; top: the regions' fill.  X: the export's staging buffer, table pair
 * and events (the calls that use it synchronise) */
struct ll_keyframes {
    ll_ctx *ctx = nullptr;
    int max_frames = 0;
    long long cap[2] = {0, 0}, top[2] = {0, 0};
    float4 *pool = nullptr;
    std::vector<ll_keyframe_info> tab;
    LLMapExport X;
    std::string err;
    unsigned long long n_reset = 0;               /* ll_keyframes_reset calls: what an ll_visibility's counters were made under */
    float4 *region(int w) const { return pool + (w ? cap[0] : 0); }
};
/* visibility (ll_visibility.hip): per pool point of ONE store two bytes (through, hit) at the point's pool index (the surf region
 * begins at cap[0]), max_images raw and eroded range images, the table pair of a run's upload (X), the events around the three
 * launches; last: the store ids of the last run's listed frames by list position; epoch: kf->n_reset when the counters were made */
struct ll_visibility {
    ll_ctx *ctx = nullptr;
    ll_keyframes *kf = nullptr;
    ll_visibility_params p;
    unsigned long long epoch = 0;
    unsigned char *d_cnt = nullptr;
    float *d_raw = nullptr, *d_img = nullptr;
    LLMapExport X;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<int> last;
    double ms[3] = {0.0, 0.0, 0.0};               /* the last run: images, erode, vote (events) */
    long long counts[3] = {0, 0, 0};              /* listed frames, their points, ordered frame pairs */
    std::string err;
};
/* correlative BEV matching (ll_bev.hip): ONE device buffer grown to a call's need -- the ops' target grids, the query counts behind
 * them (one fill zeroes both), the peak records, the score volume, the query list --, the table pair of a call's upload (X), the
 * events around the three launches, and what ll_bev_volume / ll_bev_grid need of the last successful call; epoch: kf->n_reset at
 * create / ll_bev_reset */
struct ll_bev {
    ll_ctx *ctx = nullptr;
    ll_keyframes *kf = nullptr;
    ll_bev_params p;
    unsigned long long epoch = 0;
    unsigned char *d_mem = nullptr; size_t cap_mem = 0;
    size_t at_volume = 0;                         /* of the last call, in d_mem */
    std::vector<int> last_vbase, last_nyaws;      /* per op of the last call: its first yaw row in the volume, its yaws */
    LLMapExport X;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms[3] = {0.0, 0.0, 0.0};               /* the last call: prepare, score, peak (events) */
    long long counts[3] = {0, 0, 0};              /* ops, listed points, hypotheses */
    std::string err;
};
/* map alignment (ll_map_align.hip): what an aligning object keeps between calls -- one device buffer grown to the need (search
 * tables, cell-ordered dst points, flat src stacks, per-op fit results, residual blocks and partial sums), the events around the
 * stages (two more per outer iteration), the last call's figures */
struct LLMapAlign {
    unsigned char *d_mem = nullptr; size_t cap_mem = 0;
    std::vector<hipEvent_t> ev;
    double ms[4] = {0.0, 0.0, 0.0, 0.0};          /* the last align: build, search + fit, evaluate + solve, fit record (events) */
    long long counts[3] = {0, 0, 0};              /* stack points, map points, residual blocks at the end */
};

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
    bool has_frame = false;                       /* a frame has run since create / reset / import: the stack clouds are one frame's (ll_keyframes) */
};

#define CM_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) { cm->err = std::string(#call) + ": " + hipGetErrorString(e_); return LL_ERR_HIP; } \
    } while (0)

/* ll_cubemap.hip: a compaction's copies (cm_commit's moves) of type w, out of the pool that was current into the one that is */
void cm_run_moves(ll_cubemap *cm, int w, const std::vector<CmPiece> &moves);

#define LL_HIDDEN __attribute__((visibility("hidden")))
/* ll_visibility.hip, for the filtered keyframe insert: may v's counters be read for kf's points?  LL_OK, or LL_ERR_ARG (another
 * store) / LL_ERR_STATE (the store was reset since) with *why filled */
LL_HIDDEN int llvis_check(const ll_visibility *v, const ll_keyframes *kf, std::string *why);
/* ll_keyframes.hip, for ll_drives.hip: room for n_frames more frames of at most max_pts[w] points each?  LL_OK or LL_ERR_CAPACITY (kf->err set) */
LL_HIDDEN int llkf_room(ll_keyframes *kf, int n_frames, const int max_pts[2]);
/* ll_map_export.hip: the tile size of this call; the segments of one map in output order (returns its points; segs == nullptr:
 * sizes only); the single map's table upload; the gather + copy + the one synchronisation; the last call's figures */
LL_HIDDEN int llx_tile();
LL_HIDDEN long long llx_segments(const ll_cubemap *cm, int which, long long dst0, int tile_points, unsigned long long *tile, std::vector<LLExpSeg> *segs);
LL_HIDDEN const void *llx_stage_bytes(LLMapExport &X, const void *data, size_t bytes, hipStream_t st, std::string &err);
LL_HIDDEN const LLExpSeg *llx_stage(LLMapExport &X, const std::vector<LLExpSeg> &segs, hipStream_t st, std::string &err);
LL_HIDDEN int llx_gather(LLMapExport &X, ll_ctx *ctx, const LLExpSeg *d_segs, size_t nseg, unsigned long long ntiles, long long total, size_t limit,
                         int tile_points, ll_point *out, std::string &err);
LL_HIDDEN void llx_free(LLMapExport &X);
LL_HIDDEN void llx_timing(const LLMapExport &X, double *ms3, long long *counts3);

/* map import (ll_map_export.hip), the export's inverse: one non-empty cloud of the input.  src: its first point in the input;
 * dst: where it goes (a pool, or a feature cloud of a slot); tile0: the tiles of the segments before it */
struct LLImpSeg { float4 *dst; long long src; int cnt; unsigned tile0; };
/* lane checkpoints (ll_drives.hip): what the pack launch reads of one lane beyond plain segments -- the ring-strided less-flat
 * cloud of its previous-row slot (lflat == nullptr: the cloud is contiguous and went in as a segment) and the lane's state:
 * the slot's pose, d_odom, d_m2o [7] each and fidx, 22 doubles = LL_CK_STATE_PTS points at dst_state.  Offsets in points.
 * bad: set to 1 when the rings' prefix table does not add up to n_lflat, the size the host planned the record with. */
#define LL_CK_STATE_PTS 11
struct LLCkRec { const float4 *lflat; const int *lf_pre; long long dst_lflat; int n_lflat, ring_cap; const double *pose, *odom, *m2o; const int *fidx; long long dst_state; int *bad; };

/* ll_map_export.hip, import side.  llx_import_check: the host-side refusals of one map's layout (LL_ERR_ARG / LL_ERR_CAPACITY, err
 * filled; n_points: what counts must add up to, < 0: not checked); llx_import_segments: its non-empty clouds in input order from
 * point src0 on, each into pool 0 of its type, back to back in cube order (no table changes); llx_import_commit: the map's
 * tables as ll_cubemaps_reset leaves them, then the imported layout; llx_reserve: the staging buffer grown to n points;
 * llx_scatter: the upload of n_up points from host memory (up == nullptr: none) and the one scatter launch over src -- no
 * synchronisation; llx_pack: the export gather's launch with the checkpoint records beside the tiles, into dst -- no copy, no
 * synchronisation */
LL_HIDDEN bool llx_is_device(const void *p);
LL_HIDDEN int llx_import_check(const ll_cubemap *cm, const int *cen3, const int *counts, const int *valid, int n_valid, long long n_points, std::string &err);
LL_HIDDEN void llx_import_segments(const ll_cubemap *cm, const int *counts, long long src0, int tile_points, unsigned long long *tile, std::vector<LLImpSeg> *segs);
LL_HIDDEN void llx_import_commit(ll_cubemap *cm, const int *cen3, const int *counts, const int *valid, int n_valid);
LL_HIDDEN float4 *llx_reserve(LLMapExport &X, size_t n, std::string &err);
LL_HIDDEN int llx_scatter(ll_ctx *ctx, const LLImpSeg *d_segs, size_t nseg, unsigned long long ntiles, float4 *src, const void *up, size_t n_up, int tile_points, std::string &err);
LL_HIDDEN int llx_pack(ll_ctx *ctx, const LLExpSeg *d_segs, size_t nseg, unsigned long long ntiles, const LLCkRec *d_rec, int nrec, int R, int tile_points, float4 *dst, std::string &err);

/* ll_cubemaps.hip's internals that ll_drives.hip drives (not exported from the library): a frame opens with llcms_begin (the
 * staging arena of the call), may stage tables through it, and maps from the guesses the caller left in llcms_dev_pose [S][7] */
LL_HIDDEN void llcms_begin(ll_cubemaps *cms);
LL_HIDDEN void *llcms_stage(ll_cubemaps *cms, const void *src, size_t bytes);
LL_HIDDEN double *llcms_dev_pose(ll_cubemaps *cms);
LL_HIDDEN long long llcms_syncs(const ll_cubemaps *cms);
LL_HIDDEN const std::string &llcms_err(const ll_cubemaps *cms);
/* for the lane checkpoints: lane q's map, the export's staging state, a table staged straight to dst, one more counted sync */
LL_HIDDEN ll_cubemap *llcms_map(ll_cubemaps *cms, int q);
LL_HIDDEN LLMapExport &llcms_export_state(ll_cubemaps *cms);
LL_HIDDEN void *llcms_stage_to(ll_cubemaps *cms, const void *src, size_t bytes, void *dst);
LL_HIDDEN int llcms_sync(ll_cubemaps *cms);
/* for the map merge (ll_map_merge.hip): the number of maps, the two leaf sizes, the merge's buffers, last_error set and rc handed
 * back, one more counted synchronisation (the voxel filter's read-back) */
LL_HIDDEN int llcms_size(const ll_cubemaps *cms);
LL_HIDDEN const float *llcms_leaf(const ll_cubemaps *cms);
LL_HIDDEN LLMapMerge &llcms_merge_state(ll_cubemaps *cms);
LL_HIDDEN int llcms_fail(ll_cubemaps *cms, int rc, const std::string &msg);
LL_HIDDEN void llcms_count_sync(ll_cubemaps *cms);
LL_HIDDEN void llmm_free(LLMapMerge &G);
/* for the map alignment (ll_map_align.hip): its buffers */
LL_HIDDEN LLMapAlign &llcms_align_state(ll_cubemaps *cms);
LL_HIDDEN void llal_free(LLMapAlign &A);
LL_HIDDEN int llcms_process_slots_dev(ll_cubemaps *cms, const int *slots, double *pose_w7, int *ran, const void *extra_dev, void *extra_host,
                                      size_t extra_bytes, ScanHdr *hdr_out);
/* the same for ll_cubemaps_localize_slots (map_of [S], read for the running sequences; fit [S], rows of the running sequences) */
LL_HIDDEN int llcms_localize_slots_dev(ll_cubemaps *cms, const int *slots, const int *map_of, double *pose_w7, int *ran, ll_localize_fit *fit,
                                       ll_pose_info *info /* [S], may be NULL: rows of the running sequences */, const void *extra_dev, void *extra_host, size_t extra_bytes, ScanHdr *hdr_out);
/* ll_localize.hip: one k_cms_fit workgroup per view; view v's record goes to d_fit[(views[v].pose - d_pose0) / 7] */
LL_HIDDEN void ll_launch_cms_fit(const LLMapView *d_views, int n_views, const double *d_pose0, ll_localize_fit *d_fit, hipStream_t st);
/* behind it: one k_cms_info workgroup per view; the record goes to d_info[the same index] and reads d_fit[it] */
LL_HIDDEN void ll_launch_cms_info(const LLMapView *d_views, int n_views, const double *d_pose0, const ll_localize_fit *d_fit, ll_pose_info *d_info, hipStream_t st);
