/*
 * ll_cubemaps.h -- what ll_cubemaps.hip (S cube maps side by side) shares with the translation units that work on its maps
 * (ll_drives.hip, ll_map_merge.hip, ll_map_align.hip, ll_keyframes.hip, ll_localize.hip): the workspaces the merge and the
 * alignment keep inside an ll_cubemaps, and its internal llcms_* interface (not exported from the library).
 */
#pragma once
#include "ll_cubemap.h"

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
/* map alignment (ll_map_align.hip): what an aligning object keeps between calls -- one device buffer grown to the need (search
 * tables, cell-ordered dst points, flat src stacks, per-op fit results, residual blocks and partial sums), the events around the
 * stages (two more per outer iteration), the last call's figures */
struct LLMapAlign {
    unsigned char *d_mem = nullptr; size_t cap_mem = 0;
    std::vector<hipEvent_t> ev;
    double ms[4] = {0.0, 0.0, 0.0, 0.0};          /* the last align: build, search + fit, evaluate + solve, fit record (events) */
    long long counts[3] = {0, 0, 0};              /* stack points, map points, residual blocks at the end */
};
LL_HIDDEN void llmm_free(LLMapMerge &G);
LL_HIDDEN void llal_free(LLMapAlign &A);

/* ll_cubemaps.hip's internals that ll_drives.hip drives: a frame opens with llcms_begin (the staging arena of the call), may stage
 * tables through it, and maps from the guesses the caller left in llcms_dev_pose [S][7] */
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
/* for the map alignment (ll_map_align.hip): its buffers */
LL_HIDDEN LLMapAlign &llcms_align_state(ll_cubemaps *cms);
LL_HIDDEN int llcms_process_slots_dev(ll_cubemaps *cms, const int *slots, double *pose_w7, int *ran, const void *extra_dev, void *extra_host,
                                      size_t extra_bytes, ScanHdr *hdr_out);
/* the same for ll_cubemaps_localize_slots (map_of [S], read for the running sequences; fit [S], rows of the running sequences) */
LL_HIDDEN int llcms_localize_slots_dev(ll_cubemaps *cms, const int *slots, const int *map_of, double *pose_w7, int *ran, ll_localize_fit *fit,
                                       ll_pose_info *info /* [S], may be NULL: rows of the running sequences */, const void *extra_dev, void *extra_host, size_t extra_bytes, ScanHdr *hdr_out);
/* ll_localize.hip: one k_cms_fit workgroup per view; view v's record goes to d_fit[(views[v].pose - d_pose0) / 7] */
LL_HIDDEN void ll_launch_cms_fit(const LLMapView *d_views, int n_views, const double *d_pose0, ll_localize_fit *d_fit, hipStream_t st);
/* behind it: one k_cms_info workgroup per view; the record goes to d_info[the same index] and reads d_fit[it] */
LL_HIDDEN void ll_launch_cms_info(const LLMapView *d_views, int n_views, const double *d_pose0, const ll_localize_fit *d_fit, ll_pose_info *d_info, hipStream_t st);
