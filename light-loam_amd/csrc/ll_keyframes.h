/*
 * ll_keyframes.h -- the keyframe store (ll_keyframes.hip) and the objects that follow it and read its pool (ll_visibility.hip,
 * ll_bev.hip, ll_entropy.hip) as the translation units that use them see them (ll_map_merge.hip inserts keyframes, ll_drives.hip
 * captures them).  The store and every follower keep an LLMapExport for their table uploads; nothing here needs the cube maps.
 * The lists of frames that the followers and the insert take are ll_kf_list.h.
 */
#pragma once
#include "ll_internal.h"
#include "ll_kf_list.h"
#include "ll_map_export.h"

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
    unsigned long long n_reset = 0;               /* ll_keyframes_reset calls: what a follower's state (visibility counters, the last BEV call, the last entropy run) was made under */
    float4 *region(int w) const { return pool + (w ? cap[0] : 0); }
};

/* a device range to the host (LLKfReader::read): bytes == 0 or src == nullptr: not copied; dst == nullptr: left in the scratch */
struct LLKfRange { const void *src; size_t bytes; void *dst; };
/* what every object that follows ONE store keeps: the store, epoch: kf->n_reset when the object last followed it (create and the
 * object's reset), the table pair of a call's upload (X), the last error */
struct LLKfReader {
    ll_ctx *ctx = nullptr;
    ll_keyframes *kf = nullptr;
    unsigned long long epoch = 0;
    LLMapExport X;
    std::string err;
    void follow(ll_keyframes *store) { ctx = store->ctx; kf = store; epoch = store->n_reset; }
    int fail(int rc, const std::string &msg) { err = msg; return rc; }
    int stale(const char *msg) { return epoch == kf->n_reset ? LL_OK : fail(LL_ERR_STATE, msg); }   /* the store was reset since */
    /* the ranges to the host through the page-locked scratch, range r at the sum of the sizes before it, with ONE synchronisation;
     * *pin: the scratch, for what a range left there.  who: the messages' prefix */
    LL_HIDDEN int read(const char *who, const LLKfRange *ranges, int n, const unsigned char **pin = nullptr);
    LL_HIDDEN void release();                     /* destroy: the stream drained, X freed */
};
/* create has no object yet: its errors go to the store */
static inline int llkf_create_err(ll_keyframes *kf, int rc, const std::string &msg) { kf->err = msg; return rc; }
/* the *_timing calls: the last run's ms[n] and counts[n] out, either may be NULL */
static inline int llkf_timing(const double *ms, const long long *counts, int n, double *ms_out, long long *counts_out)
{
    if (ms_out) for (int k = 0; k < n; ++k) ms_out[k] = ms[k];
    if (counts_out) for (int k = 0; k < n; ++k) counts_out[k] = counts[k];
    return LL_OK;
}

/* visibility (ll_visibility.hip): per pool point of ONE store two bytes (through, hit) at the point's pool index (the surf region
 * begins at cap[0]), max_images raw and eroded range images, the events around the three launches; last: the store ids of the last
 * run's listed frames by list position; epoch: when the counters were made */
struct ll_visibility : LLKfReader {
    ll_visibility_params p;
    unsigned char *d_cnt = nullptr;
    float *d_raw = nullptr, *d_img = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<int> last;
    double ms[3] = {0.0, 0.0, 0.0};               /* the last run: images, erode, vote (events) */
    long long counts[3] = {0, 0, 0};              /* listed frames, their points, ordered frame pairs */
};
/* correlative BEV matching (ll_bev.hip): ONE device buffer grown to a call's need -- the ops' target grids, the query counts behind
 * them (one fill zeroes both), the peak records, the score volume, the query list --, the events around the three launches, and
 * what ll_bev_volume / ll_bev_grid need of the last successful call */
struct ll_bev : LLKfReader {
    ll_bev_params p;
    unsigned char *d_mem = nullptr; size_t cap_mem = 0;
    size_t at_volume = 0;                         /* of the last call, in d_mem */
    std::vector<int> last_vbase, last_nyaws;      /* per op of the last call: its first yaw row in the volume, its yaws */
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms[3] = {0.0, 0.0, 0.0};               /* the last call: prepare, score, peak (events) */
    long long counts[3] = {0, 0, 0};              /* ops, listed points, hypotheses */
};

/* ll_visibility.hip, for the filtered keyframe insert: may v's counters be read for kf's points?  LL_OK, or LL_ERR_ARG (another
 * store) / LL_ERR_STATE (the store was reset since) with *why filled */
LL_HIDDEN int llvis_check(const ll_visibility *v, const ll_keyframes *kf, std::string *why);
/* ll_keyframes.hip, for ll_drives.hip: room for n_frames more frames of at most max_pts[w] points each?  LL_OK or LL_ERR_CAPACITY (kf->err set) */
LL_HIDDEN int llkf_room(ll_keyframes *kf, int n_frames, const int max_pts[2]);
