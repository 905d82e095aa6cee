/*
 * ll_map_export.h -- the tiled copies of ll_map_export.hip as the other translation units see them: the segment types of the map
 * export, the map import and the lane checkpoints, the state an exporting object keeps between calls, and the llx_* functions
 * (not exported from the library).  The tile vocabulary is ll_tiles.h.
 */
#pragma once
#include "ll_internal.h"
#include "ll_tiles.h"

struct ll_cubemap;

/* map export: one non-empty cloud of the output.  dst: its first point in the output; tile0: the tiles of the segments before it */
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

/* the tile size of this call (an LLTiler's `per`); the segments of one map in output order, numbered by T (returns its points;
 * T == nullptr: sizes only, segs is not touched); the single map's table upload; the gather + copy + the one synchronisation; the
 * last call's figures */
LL_HIDDEN int llx_tile();
LL_HIDDEN long long llx_segments(const ll_cubemap *cm, int which, long long dst0, LLTiler *T, std::vector<LLExpSeg> *segs);
LL_HIDDEN const void *llx_stage_bytes(LLMapExport &X, const void *data, size_t bytes, hipStream_t st, std::string &err);
LL_HIDDEN const LLExpSeg *llx_stage(LLMapExport &X, const std::vector<LLExpSeg> &segs, hipStream_t st, std::string &err);
LL_HIDDEN int llx_gather(LLMapExport &X, ll_ctx *ctx, const LLExpSeg *d_segs, size_t nseg, unsigned long long ntiles, long long total, size_t limit,
                         int tile_points, ll_point *out, std::string &err);
LL_HIDDEN void llx_free(LLMapExport &X);
LL_HIDDEN void llx_timing(const LLMapExport &X, double *ms3, long long *counts3);

/* map import, the export's inverse: one non-empty cloud of the input.  src: its first point in the input; dst: where it goes (a
 * pool, or a feature cloud of a slot); tile0: the tiles of the segments before it */
struct LLImpSeg { float4 *dst; long long src; int cnt; unsigned tile0; };
/* lane checkpoints (ll_drives.hip): what the pack launch reads of one lane beyond plain segments -- the ring-strided less-flat
 * cloud of its previous-row slot (lflat == nullptr: the cloud is contiguous and went in as a segment) and the lane's state:
 * the slot's pose, d_odom, d_m2o [7] each and fidx, 22 doubles = LL_CK_STATE_PTS points at dst_state.  Offsets in points.
 * bad: set to 1 when the rings' prefix table does not add up to n_lflat, the size the host planned the record with. */
#define LL_CK_STATE_PTS 11
struct LLCkRec { const float4 *lflat; const int *lf_pre; long long dst_lflat; int n_lflat, ring_cap; const double *pose, *odom, *m2o; const int *fidx; long long dst_state; int *bad; };

/* the import side.  llx_import_check: the host-side refusals of one map's layout (LL_ERR_ARG / LL_ERR_CAPACITY, err filled;
 * n_points: what counts must add up to, < 0: not checked); llx_import_segments: its non-empty clouds in input order from point src0
 * on, numbered by T, each into pool 0 of its type, back to back in cube order (no table changes); llx_import_commit: the map's
 * tables as ll_cubemaps_reset leaves them, then the imported layout; llx_reserve: the staging buffer grown to n points;
 * llx_scatter: the upload of n_up points from host memory (up == nullptr: none) and the one scatter launch over src -- no
 * synchronisation; llx_pack: the export gather's launch with the checkpoint records beside the tiles, into dst -- no copy, no
 * synchronisation */
LL_HIDDEN bool llx_is_device(const void *p);
LL_HIDDEN int llx_import_check(const ll_cubemap *cm, const int *cen3, const int *counts, const int *valid, int n_valid, long long n_points, std::string &err);
LL_HIDDEN void llx_import_segments(const ll_cubemap *cm, const int *counts, long long src0, LLTiler &T, std::vector<LLImpSeg> *segs);
LL_HIDDEN void llx_import_commit(ll_cubemap *cm, const int *cen3, const int *counts, const int *valid, int n_valid);
LL_HIDDEN float4 *llx_reserve(LLMapExport &X, size_t n, std::string &err);
LL_HIDDEN int llx_scatter(ll_ctx *ctx, const LLImpSeg *d_segs, size_t nseg, unsigned long long ntiles, float4 *src, const void *up, size_t n_up, int tile_points, std::string &err);
LL_HIDDEN int llx_pack(ll_ctx *ctx, const LLExpSeg *d_segs, size_t nseg, unsigned long long ntiles, const LLCkRec *d_rec, int nrec, int R, int tile_points, float4 *dst, std::string &err);
