/*
 * ll_keyframes.hip -- the clouds every mapped frame contributed to its cube map (laserMapping.cpp:2103-2125: the down-sized
 * laserCloudCornerStack / laserCloudSurfStack in the sensor frame) kept on the device with the pose the frame was mapped under, so
 * that a map can be rebuilt under corrected poses (ll_cubemaps_insert_keyframes, ll_map_merge.hip).
 *
 * The store is two regions of one allocation, one per cloud type, filled back to back, and a host table: every size is known to the
 * host (a frame's stack sizes came back with its prepare), so capture and export are tables of (source, destination, count)
 * segments handed to the map export's tiled copy (ll_map_export.hip: a workgroup per 1024-point tile, the segment found by a binary
 * search, every load of a tile before its first store).  No kernel of its own.
 *   capture   ONE launch for all selected sequences and both types, device to device, no synchronisation; the table goes up through
 *             the cube maps' per-call arena, behind what the frame staged there;
 *   export    one gather into a staging buffer, one copy, one synchronisation (llx_gather).
 */
#include "ll_keyframes.h"
#include "ll_cubemaps.h"
#include "ll_pose_math.h"
#include <cmath>

static int kf_fail(ll_keyframes *kf, int rc, const std::string &msg) { kf->err = msg; return rc; }
static const char *kf_type(int w) { return w ? "surf" : "corner"; }

extern "C" int ll_keyframes_create(ll_ctx *ctx, const ll_keyframes_params *p, ll_keyframes **out)
{
    if (!ctx || !p || !out) return LL_ERR_ARG;
    *out = nullptr;
    if (p->max_frames < 1 || p->max_frames > (1 << 24) || p->cap_corner < 1 || p->cap_corner > (1ll << 30) || p->cap_surf < 1 || p->cap_surf > (1ll << 30)) {
        ctx->err = "bad keyframes parameters (max_frames in 1 .. 2^24, cap_corner / cap_surf in 1 .. 2^30)"; return LL_ERR_ARG;
    }
    LL_HIP(hipSetDevice(ctx->device));
    void *mem = nullptr;
    const size_t bytes = (size_t)(p->cap_corner + p->cap_surf) * sizeof(float4);
    if (hipMalloc(&mem, bytes) != hipSuccess) { (void)hipGetLastError(); ctx->err = "keyframes: hipMalloc failed (" + std::to_string(bytes) + " bytes)"; return LL_ERR_HIP; }
    ll_keyframes *kf = new ll_keyframes();
    kf->ctx = ctx; kf->max_frames = p->max_frames; kf->cap[0] = p->cap_corner; kf->cap[1] = p->cap_surf;
    kf->pool = (float4 *)mem;
    *out = kf;
    return LL_OK;
}

extern "C" void ll_keyframes_destroy(ll_keyframes *kf)
{
    if (!kf) return;
    if (kf->ctx) { (void)hipSetDevice(kf->ctx->device); (void)hipStreamSynchronize(kf->ctx->stream); }
    if (kf->pool) (void)hipFree(kf->pool);
    llx_free(kf->X);
    delete kf;
}

extern "C" const char *ll_keyframes_last_error(const ll_keyframes *kf) { return kf ? kf->err.c_str() : "null keyframes"; }
extern "C" int ll_keyframes_size(const ll_keyframes *kf) { return kf ? (int)kf->tab.size() : LL_ERR_ARG; }

/* the pools' contents are dead from here on: nothing reads a pool beyond the table, and what was enqueued reads in stream order */
extern "C" int ll_keyframes_reset(ll_keyframes *kf)
{
    if (!kf) return LL_ERR_ARG;
    kf->tab.clear(); kf->top[0] = kf->top[1] = 0;
    ++kf->n_reset;                                                /* what a follower (LLKfReader) kept of the old table means nothing from here on */
    return LL_OK;
}

void LLKfReader::release()
{
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    llx_free(X);
}

#define KFR_HIP(call) LL_HIP_CHECK(ll_fail, this, who, call, #call)
int LLKfReader::read(const char *who, const LLKfRange *ranges, int n, const unsigned char **pin_out)
{
    size_t total = 0;
    for (int r = 0; r < n; ++r) total += ranges[r].bytes;
    unsigned char *pin = (unsigned char *)ll_pinned_scratch(total);
    if (!pin) return fail(LL_ERR_HIP, std::string(who) + "no page-locked scratch");
    hipStream_t st = ctx->stream;
    KFR_HIP(hipSetDevice(ctx->device));
    size_t at = 0;
    for (int r = 0; r < n; at += ranges[r++].bytes)
        if (ranges[r].src && ranges[r].bytes) KFR_HIP(hipMemcpyAsync(pin + at, ranges[r].src, ranges[r].bytes, hipMemcpyDeviceToHost, st));
    KFR_HIP(hipStreamSynchronize(st));
    at = 0;
    for (int r = 0; r < n; at += ranges[r++].bytes)
        if (ranges[r].src && ranges[r].bytes && ranges[r].dst) std::memcpy(ranges[r].dst, pin + at, ranges[r].bytes);
    if (pin_out) *pin_out = pin;
    return LL_OK;
}

extern "C" int ll_keyframes_info(const ll_keyframes *kf, int id, ll_keyframe_info *info)
{
    if (!kf || !info) return LL_ERR_ARG;
    if (id < 0 || id >= (int)kf->tab.size()) return kf_fail(const_cast<ll_keyframes *>(kf), LL_ERR_ARG, "keyframes: frame " + std::to_string(id) + " is not in the store (size " + std::to_string(kf->tab.size()) + ")");
    *info = kf->tab[id];
    return LL_OK;
}

/* room for n_frames more frames that together hold need[w] points of type w? */
static int kf_room(ll_keyframes *kf, long long n_frames, const long long need[2])
{
    if ((long long)kf->tab.size() + n_frames > (long long)kf->max_frames)
        return kf_fail(kf, LL_ERR_CAPACITY, "keyframes: frames: " + std::to_string(kf->tab.size()) + " stored + " + std::to_string(n_frames) + " new, max_frames is " + std::to_string(kf->max_frames));
    for (int w = 0; w < 2; ++w)
        if (kf->top[w] + need[w] > kf->cap[w])
            return kf_fail(kf, LL_ERR_CAPACITY, std::string("keyframes: ") + kf_type(w) + ": " + std::to_string(kf->top[w]) + " points stored + " + std::to_string(need[w]) + " new, cap_" + kf_type(w) +
                                                    " is " + std::to_string(kf->cap[w]));
    return LL_OK;
}

int llkf_room(ll_keyframes *kf, int n_frames, const int max_pts[2])
{
    const long long need[2] = {(long long)n_frames * max_pts[0], (long long)n_frames * max_pts[1]};
    return kf_room(kf, n_frames, need);
}

/* the new frame's table entry, its clouds at the regions' tops */
static ll_keyframe_info kf_entry(ll_keyframes *kf, int lane, int frame, const int n[2], const double *pose)
{
    ll_keyframe_info e;
    e.lane = lane; e.frame_index = frame;
    for (int w = 0; w < 2; ++w) { e.n[w] = n[w]; e.offset[w] = kf->top[w]; kf->top[w] += n[w]; }
    for (int k = 0; k < 7; ++k) e.pose_w7[k] = pose[k];
    return e;
}

extern "C" int ll_keyframes_add_cubemaps(ll_keyframes *kf, ll_cubemaps *cms, const int *sel, const double *pose_w7, const int *lane_tag, const int *frame_tag, int *first_id)
{
    if (!kf) return LL_ERR_ARG;
    if (!cms || !sel || !pose_w7) return kf_fail(kf, LL_ERR_ARG, "keyframes: cms, sel or pose_w7 is NULL");
    const int S = llcms_size(cms);
    if (llcms_map(cms, 0)->ctx != kf->ctx) return kf_fail(kf, LL_ERR_ARG, "keyframes: the cube maps belong to another context");
    /* ---- every refusal before anything is enqueued or the table changes */
    long long n_new = 0, need[2] = {0, 0};
    for (int q = 0; q < S; ++q) {
        if (sel[q] != 0 && sel[q] != 1) return kf_fail(kf, LL_ERR_ARG, "keyframes: sequence " + std::to_string(q) + ": sel must be 0 or 1");
        if (!sel[q]) continue;
        if (!ll_finite_n(pose_w7 + (size_t)q * 7, 7)) return kf_fail(kf, LL_ERR_ARG, "keyframes: sequence " + std::to_string(q) + ": non-finite pose");
        const ll_cubemap *cm = llcms_map(cms, q);
        if (cm->broken) return kf_fail(kf, LL_ERR_STATE, "keyframes: sequence " + std::to_string(q) + ": unusable, an earlier update failed half-way");
        if (!cm->has_frame) return kf_fail(kf, LL_ERR_STATE, "keyframes: sequence " + std::to_string(q) + " has run no frame since create / reset / import");
        ++n_new;
        for (int w = 0; w < 2; ++w) need[w] += cm->map->M.n_stk[w];
    }
    if (first_id) *first_id = n_new ? (int)kf->tab.size() : -1;
    if (n_new == 0) return LL_OK;
    int rc = kf_room(kf, n_new, need); if (rc) return rc;
    /* ---- the segments: sequence by sequence, corner then surf, each to the top of its region (offsets from the pool's base) */
    LLTiler T{llx_tile()};
    std::vector<LLExpSeg> segs;
    long long at[2] = {kf->top[0], kf->top[1]};
    for (int q = 0; q < S; ++q) {
        if (!sel[q]) continue;
        const ll_map *m = llcms_map(cms, q)->map;
        for (int w = 0; w < 2; ++w) {
            const int cnt = m->M.n_stk[w];
            if (cnt <= 0) continue;
            segs.push_back({m->d_stk[w], (w ? kf->cap[0] : 0) + at[w], cnt, T.take(cnt)});
            at[w] += cnt;
        }
    }
    if (!segs.empty()) {
        if (hipSetDevice(kf->ctx->device) != hipSuccess) return kf_fail(kf, LL_ERR_HIP, "keyframes: hipSetDevice failed");
        const LLExpSeg *d_segs = (const LLExpSeg *)llcms_stage(cms, segs.data(), segs.size() * sizeof(LLExpSeg));
        if (!d_segs) return kf_fail(kf, LL_ERR_HIP, "keyframes: " + llcms_err(cms));
        rc = llx_pack(kf->ctx, d_segs, segs.size(), T.next, nullptr, 0, 0, T.per, kf->pool, kf->err);
        if (rc) return rc;
    }
    for (int q = 0; q < S; ++q) {
        if (!sel[q]) continue;
        const ll_map *m = llcms_map(cms, q)->map;
        kf->tab.push_back(kf_entry(kf, lane_tag ? lane_tag[q] : q, frame_tag ? frame_tag[q] : -1, m->M.n_stk, pose_w7 + (size_t)q * 7));
    }
    return LL_OK;
}

extern "C" int ll_keyframes_add_points(ll_keyframes *kf, const ll_point *corner, int n_corner, const ll_point *surf, int n_surf, const double *pose_w7, int *id)
{
    if (!kf) return LL_ERR_ARG;
    if (!pose_w7 || n_corner < 0 || n_surf < 0 || (n_corner > 0 && !corner) || (n_surf > 0 && !surf)) return kf_fail(kf, LL_ERR_ARG, "keyframes: NULL cloud or pose, or a negative size");
    if (!ll_finite_n(pose_w7, 7)) return kf_fail(kf, LL_ERR_ARG, "keyframes: non-finite pose");
    const int n[2] = {n_corner, n_surf};
    const long long need[2] = {n_corner, n_surf};
    int rc = kf_room(kf, 1, need); if (rc) return rc;
    const ll_point *src[2] = {corner, surf};
    hipStream_t st = kf->ctx->stream;
    hipError_t e = hipSetDevice(kf->ctx->device);
    for (int w = 0; w < 2 && e == hipSuccess; ++w)
        if (n[w] > 0) e = hipMemcpyAsync(kf->region(w) + kf->top[w], src[w], (size_t)n[w] * sizeof(float4), llx_is_device(src[w]) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                    /* the caller's clouds may go away */
    if (e != hipSuccess) return kf_fail(kf, LL_ERR_HIP, std::string("keyframes: upload: ") + hipGetErrorString(e));
    if (id) *id = (int)kf->tab.size();
    kf->tab.push_back(kf_entry(kf, -1, -1, n, pose_w7));
    return LL_OK;
}

extern "C" int ll_keyframes_export(ll_keyframes *kf, int first, int count, ll_point *points_out, long long *offsets_out)
{
    if (!kf) return LL_ERR_ARG;
    if (!offsets_out) return kf_fail(kf, LL_ERR_ARG, "keyframes: offsets_out is NULL");
    if (first < 0 || count < 0 || (long long)first + count > (long long)kf->tab.size())
        return kf_fail(kf, LL_ERR_ARG, "keyframes: frames " + std::to_string(first) + " .. + " + std::to_string(count) + " are not in the store (size " + std::to_string(kf->tab.size()) + ")");
    LLTiler T{llx_tile()};
    std::vector<LLExpSeg> segs;
    long long at = 0;
    for (int f = 0; f < count; ++f) {
        const ll_keyframe_info &e = kf->tab[first + f];
        for (int w = 0; w < 2; ++w) {
            offsets_out[2 * f + w] = at;
            if (e.n[w] > 0 && points_out) segs.push_back({kf->region(w) + e.offset[w], at, e.n[w], T.take(e.n[w])});
            at += e.n[w];
        }
    }
    offsets_out[2 * count] = at;
    if (!points_out || at == 0) return LL_OK;
    if (!T.fits()) return kf_fail(kf, LL_ERR_CAPACITY, "keyframes: too many tiles for one launch");
    if (hipSetDevice(kf->ctx->device) != hipSuccess) return kf_fail(kf, LL_ERR_HIP, "keyframes: hipSetDevice failed");
    const LLExpSeg *d_segs = llx_stage(kf->X, segs, kf->ctx->stream, kf->err);
    if (!d_segs) return LL_ERR_HIP;
    return llx_gather(kf->X, kf->ctx, d_segs, segs.size(), T.next, at, (size_t)(kf->cap[0] + kf->cap[1]), T.per, points_out, kf->err);
}
