/*
 * ll_drives.hip -- whole drives side by side: S lanes, each running one drive at a time through registration, odometry and
 * mapping -- the chain of ll_odometry_kitti with mapping = 1 (extract, ll_odometry_frames, WorldPose, LaserMapping's
 * transformAssociateToMap / process_slot / transformUpdate) for every lane in one set of launches per stage.
 * The lanes' pose state lives on the device, so a step adds no host synchronisation to those of its cube-map frame:
 *   ll_extract_batch over the row, ll_odometry_sequences (one row, RUN lanes), k_drives_associate (world pose, :830-831, and
 *   transformAssociateToMap, laserMapping.cpp:113-117, straight into the cube maps' pose array), the cube-map frame from those
 *   guesses (ll_cubemaps.hip: they come to the host with the slot headers it reads back anyway), k_drives_update
 *   (transformUpdate, :119-123) and, with keep_registered, k_drives_register (pointAssociateToMap of laserCloud, :125-133).
 * The pose arithmetic is ll_pose_math.h's Eigen form -- ll_qmul, ll_rotate, ll_pose_compose: lightloam::WorldPose::compose and
 * LaserMapping::qmul / qrot (lightloam_host.hpp) in their operation order, in double; the library is built with -ffp-contract=off,
 * so it is bit for bit the host's.
 * A lane may instead localise against another lane's frozen map (ll_drives_set_localize): the same chain with the read-only frame
 * of ll_cubemaps_localize_slots in place of the mapping frame; a step runs the mapping lanes' frame, then the localising lanes',
 * and refuses beforehand any command set in which one would write what the other reads.
 */
#include "ll_cubemaps.h"
#include "ll_keyframes.h"
#include "ll_factor_math.h"
#include <cmath>

/* per lane: odom [S][7] = q_w_curr, t_w_curr (laserOdometry); m2o [S][7] = q_wmap_wodom, t_wmap_wodom (laserMapping);
 * start [S][7] = what START sets m2o to (ll_drives_set_localize; identity rows for mapping lanes) */
__global__ __launch_bounds__(64) void k_drives_associate(double *vpose, int first, int S, const int *cmd, const double *pose0, const double *start,
                                                          double *odom, double *m2o, int *fidx, double *map_pose)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= S) return;
    const int c = cmd[q];
    if (c == LL_DRIVE_IDLE) return;
    double *W = odom + (size_t)q * 7, *M = m2o + (size_t)q * 7, *slot_pose = vpose + (size_t)(first + q) * 7;
    if (c == LL_DRIVE_START) {
        for (int k = 0; k < 7; ++k) { W[k] = k == 3 ? 1.0 : 0.0; M[k] = start[(size_t)q * 7 + k]; }   /* identity for a mapping lane; where a localising lane's drive begins in the map */
        for (int k = 0; k < 7; ++k) slot_pose[k] = pose0[(size_t)q * 7 + k];     /* the warm start of frame 1 (:61-65) */
        fidx[q] = 0;
    } else {                                                                      /* WorldPose::compose (:830-831), kept as the host spells it: W is updated in place, t before q */
        double r[3];
        ll_rotate(W, slot_pose + 4, r);
        for (int k = 0; k < 3; ++k) W[4 + k] += r[k];
        ll_qmul(W, slot_pose, W);
        fidx[q] += 1;
    }
    ll_pose_compose(M, W, map_pose + (size_t)q * 7);                              /* transformAssociateToMap (:113-117) */
}

/* transformUpdate (:119-123) from the mapped parameters[] of every running lane */
__global__ __launch_bounds__(64) void k_drives_update(int S, const int *cmd, const double *odom, double *m2o, const double *map_pose)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= S || cmd[q] == LL_DRIVE_IDLE) return;
    const double *qc = odom + (size_t)q * 7, *tc = qc + 4, *P = map_pose + (size_t)q * 7;
    double *M = m2o + (size_t)q * 7;
    const double n2 = qc[0] * qc[0] + qc[1] * qc[1] + qc[2] * qc[2] + qc[3] * qc[3];
    const double inv[4] = {-qc[0] / n2, -qc[1] / n2, -qc[2] / n2, qc[3] / n2};
    double qm[4], r[3];
    ll_qmul(P, inv, qm);
    ll_rotate(qm, tc, r);
    for (int k = 0; k < 4; ++k) M[k] = qm[k];
    for (int k = 0; k < 3; ++k) M[4 + k] = P[4 + k] - r[k];
}

/* pointAssociateToMap (:125-133) of laserCloud for every lane of the table: block (x, y, z) moves points [256 x, 256 x + 256) of
 * ring y of lane lanes[z] -- read in place from the ring-strided cloud (k_cloud_flatten's addressing), written in laserCloud
 * order into the lane's row of out (stride CS); one float4 in, one float4 out per thread */
struct DrvReg { int lane, slot; };
__global__ __launch_bounds__(256) void k_drives_register(LLView V, const DrvReg *lanes, const double *map_pose, float4 *out)
{
    const DrvReg L = lanes[blockIdx.z];
    const int r = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int *ring_off = V.ring_off + (size_t)L.slot * (V.R + 1);
    const int off = ring_off[r], n = min(ring_off[r + 1] - off, V.ring_cap);
    if (i >= n || off + i >= V.CS || off < 0) return;
    const float4 p = V.cloud[(size_t)L.slot * V.CS + (size_t)r * V.ring_cap + i];
    float sx, sy, sz;
    ll_map_to_world(map_pose + (size_t)L.lane * 7, p, sx, sy, sz);
    out[(size_t)L.lane * V.CS + off + i] = make_float4(sx, sy, sz, p.w);
}

/* ll_drives_correct: the map-to-odom pose of every selected lane left-multiplied by its C (q_C, t_C), spelled as
 * transformAssociateToMap spells its products (ll_pose_compose): q' = q_C * q_m2o, t' = R(q_C) t_m2o + t_C */
__global__ __launch_bounds__(64) void k_drives_correct(int S, const int *sel, const double *C, double *m2o)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= S || !sel[q]) return;
    const double *Cq = C + (size_t)q * 7;
    double *M = m2o + (size_t)q * 7;
    ll_pose_compose(Cq, M, M);
}

/* ll_drives_restore: the state of one record out of the uploaded blob -- the slot's pose and header (as ll_upload_features
 * leaves one), the lane's two poses and frame counter */
struct DrvRestore { long long src_state; int slot, lane; ScanHdr hdr; };
__global__ __launch_bounds__(64) void k_drives_restore(const DrvRestore *tab, const float4 *src, double *vpose, double *odom, double *m2o, int *fidx, ScanHdr *hdr)
{
    const DrvRestore R = tab[blockIdx.x];
    const double *in = (const double *)(src + R.src_state);
    const int t = threadIdx.x;
    if (t < 7) { vpose[(size_t)R.slot * 7 + t] = in[t]; odom[(size_t)R.lane * 7 + t] = in[7 + t]; m2o[(size_t)R.lane * 7 + t] = in[14 + t]; }
    if (t == 0) { fidx[R.lane] = ((const int *)(in + 21))[0]; hdr[R.slot] = R.hdr; }
}

/* ------------------------------------------------------------------ host side */
struct DrvFeat { int n[4] = {0, 0, 0, 0}; int strided = 0; };   /* sharp, less sharp, flat, less flat; the less-flat cloud's layout */
struct ll_drives {
    ll_ctx *ctx = nullptr;
    ll_cubemaps *cms = nullptr;
    int S = 0, base = 0, n_outer = 3, keep_registered = 0;
    int map_vote_from = -1;                       /* ll_drives_set_map_vote: a mapping lane votes its plane blocks in frames with index > this; < 0: never */
    ll_keyframes *kf = nullptr; int kf_every = 1;  /* ll_drives_set_keyframes: the store every kf_every-th frame of a lane is captured into (nullptr: off) */
    int row = 0;                                  /* the row the next step reads */
    std::vector<int> ran_prev, fidx, reg_n;       /* per lane: ran on the last step, frame index of its last frame, registered points */
    std::vector<DrvFeat> feat;                    /* per lane: the feature counts of its previous-row slot (from the step's header read-back, or a restore) */
    double *d_odom = nullptr, *d_m2o = nullptr;   /* [S][7] each */
    double *d_start = nullptr;                    /* [S][7]: the map-to-odom pose START gives a lane (identity unless ll_drives_set_localize said otherwise) */
    std::vector<int> map_of;                      /* per lane: -1 maps into its own map; m >= 0 localises against lane m's map */
    std::vector<ll_localize_fit> fit;             /* per lane: the last step's fit record (zeros unless the lane localised and optimised) */
    std::vector<ll_pose_info> info; int info_on = 0;   /* ll_drives_set_info: the same for the information records; off: zeros, nothing launched */
    int *d_fidx = nullptr;                        /* [S]: the frame counter, mirrored on the device */
    int *d_ck_bad = nullptr;                      /* [1]: ll_drives_save's pack launch found a less-flat table that disagrees with its header */
    float4 *d_reg = nullptr;                      /* [S][CS] registered clouds (keep_registered) */
    std::vector<void *> allocs;
    long long syncs = 0, frames = 0;
    std::string err;
};

#define DRV_HIP(call) LL_HIP_CHECK(ll_fail, d, "", call, #call)

template <typename T>
static bool drv_alloc(ll_drives *d, T *&ptr, size_t count) { return ll_dev_alloc(d->allocs, d->err, ptr, count, true); }

extern "C" void ll_drives_destroy(ll_drives *d)
{
    if (!d) return;
    if (d->ctx) { (void)hipSetDevice(d->ctx->device); (void)hipStreamSynchronize(d->ctx->stream); }
    ll_cubemaps_destroy(d->cms);
    for (void *p : d->allocs) (void)hipFree(p);
    delete d;
}

extern "C" const char *ll_drives_last_error(const ll_drives *d) { return d ? d->err.c_str() : "null drives"; }

extern "C" int ll_drives_create(ll_ctx *ctx, const ll_drives_params *p, ll_drives **out)
{
    if (!ctx || !p || !out) return LL_ERR_ARG;
    *out = nullptr;
    const int S = p->n_lanes;
    if (S < 1 || S > 4096) { ctx->err = "n_lanes must be in 1..4096"; return LL_ERR_ARG; }
    if (p->base < 0 || (long long)p->base + 2LL * S > ctx->p.batch) { ctx->err = "slots [base, base + 2 n_lanes) do not fit in the batch"; return LL_ERR_ARG; }
    if (p->n_outer < 1 || p->n_outer > 16) { ctx->err = "n_outer out of range"; return LL_ERR_ARG; }
    if (p->keep_registered != 0 && p->keep_registered != 1) { ctx->err = "keep_registered must be 0 or 1"; return LL_ERR_ARG; }
    LL_HIP(hipSetDevice(ctx->device));
    ll_cubemaps *cms = nullptr;
    int rc = ll_cubemaps_create(ctx, S, p->line_res, p->plane_res, p->max_scan_corner, p->max_scan_surf, p->pool_points, &cms);
    if (rc) return rc;
    ll_drives *d = new ll_drives();
    d->ctx = ctx; d->cms = cms; d->S = S; d->base = p->base; d->n_outer = p->n_outer; d->keep_registered = p->keep_registered;
    d->ran_prev.assign(S, 0); d->fidx.assign(S, 0); d->reg_n.assign(S, 0); d->feat.assign(S, DrvFeat());
    d->map_of.assign(S, -1); d->fit.assign(S, ll_localize_fit()); d->info.assign(S, ll_pose_info());
    bool ok = drv_alloc(d, d->d_odom, (size_t)S * 7) && drv_alloc(d, d->d_m2o, (size_t)S * 7) && drv_alloc(d, d->d_fidx, (size_t)S) && drv_alloc(d, d->d_ck_bad, 1) &&
              drv_alloc(d, d->d_start, (size_t)S * 7);
    if (ok) {
        std::vector<double> ident((size_t)S * 7, 0.0);
        for (int q = 0; q < S; ++q) ident[(size_t)q * 7 + 3] = 1.0;
        ok = hipMemcpy(d->d_start, ident.data(), ident.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) d->err = "upload of the start poses failed";
    }
    if (ok && d->keep_registered) ok = drv_alloc(d, d->d_reg, (size_t)S * (size_t)ctx->V.CS);
    if (!ok) { ctx->err = d->err; ll_drives_destroy(d); return LL_ERR_HIP; }
    *out = d;
    return LL_OK;
}

extern "C" int ll_drives_slots(ll_drives *d, int *slots)
{
    if (!d || !slots) return LL_ERR_ARG;
    for (int q = 0; q < d->S; ++q) slots[q] = d->base + d->row * d->S + q;
    return LL_OK;
}

extern "C" ll_cubemaps *ll_drives_cubemaps(ll_drives *d) { return d ? d->cms : nullptr; }

extern "C" int ll_drives_stats(const ll_drives *d, long long *syncs, long long *frames)
{
    if (!d) return LL_ERR_ARG;
    if (syncs) *syncs = d->syncs;
    if (frames) *frames = d->frames;
    return LL_OK;
}

/* "sequence q: ..." of the cube maps -> "lane q: ..." */
static std::string drv_lane_msg(const std::string &m)
{
    const std::string pre = "sequence ";
    return m.compare(0, pre.size(), pre) == 0 ? "lane " + m.substr(pre.size()) : m;
}

/* the mapping vote of the lanes that map: frames whose per-lane index (0 at START) is > from_frame vote; from_frame < 0 switches it off for
 * every lane.  Localising lanes never vote.  Not part of a checkpoint: set it again after ll_drives_restore. */
extern "C" int ll_drives_set_map_vote(ll_drives *d, int from_frame)
{
    if (!d) return LL_ERR_ARG;
    if (from_frame < 0) {
        std::vector<int> off(d->S, 0);
        const int rc = ll_cubemaps_set_vote(d->cms, off.data());
        if (rc) { d->err = "mapping vote: " + drv_lane_msg(llcms_err(d->cms)); return rc; }
        d->map_vote_from = -1;
        return LL_OK;
    }
    /* the first switch-on of a map allocates and may refuse: now, not in the middle of a drive -- a step then only flips the switches */
    for (int q = 0; q < d->S; ++q) {
        ll_map *m = llcms_map(d->cms, q)->map;
        if (m->M.ctr) continue;
        const int rc = ll_map_set_vote(m, 1);
        if (rc) { d->err = "mapping vote: lane " + std::to_string(q) + ": " + m->err; return rc; }
        (void)ll_map_set_vote(m, 0);
    }
    d->map_vote_from = from_frame;
    return LL_OK;
}

/* everything after the argument checks: a failure loses the step for every lane in run */
static int drv_run(ll_drives *d, const int *cmd, const std::vector<double> &p0, std::vector<double> &odom, std::vector<double> &mapped, std::vector<int> &ran)
{
    ll_ctx *ctx = d->ctx;
    hipStream_t st = ctx->stream;
    const int S = d->S, first = d->base + d->row * S;
    int qmin = S, qmax = -1, n_run_odo = 0;
    for (int q = 0; q < S; ++q)
        if (cmd[q] != LL_DRIVE_IDLE) { qmin = std::min(qmin, q); qmax = q; n_run_odo += cmd[q] == LL_DRIVE_RUN; }
    llcms_begin(d->cms);
    const int *d_cmd = (const int *)llcms_stage(d->cms, cmd, (size_t)S * sizeof(int));
    const double *d_p0 = (const double *)llcms_stage(d->cms, p0.data(), p0.size() * sizeof(double));
    if (!d_cmd || !d_p0) { d->err = llcms_err(d->cms); return LL_ERR_HIP; }
    int rc = ll_extract_batch(ctx, first + qmin, qmax - qmin + 1);                     /* scanRegistration */
    if (rc) { d->err = "extract: " + ctx->err; return rc; }
    if (n_run_odo > 0) {                                                                /* laserOdometry, one row */
        const ll_seq_layout L = {d->base, S, 2};
        std::vector<int> rows(S, 0), fi(S, 1);
        for (int q = 0; q < S; ++q)
            if (cmd[q] == LL_DRIVE_RUN) { rows[q] = 1; fi[q] = d->fidx[q] + 1; }
        rc = ll_odometry_sequences(ctx, &L, d->row, 1, rows.data(), fi.data(), nullptr, d->n_outer, nullptr, nullptr);
        if (rc) { d->err = "odometry: " + ctx->err; return rc; }
    }
    double *d_map_pose = llcms_dev_pose(d->cms);
    const unsigned nb = (unsigned)((S + 63) / 64);
    hipLaunchKernelGGL(k_drives_associate, dim3(nb), dim3(64), 0, st, ctx->V.pose, first, S, d_cmd, d_p0, (const double *)d->d_start, d->d_odom, d->d_m2o, d->d_fidx, d_map_pose);
    DRV_HIP(hipGetLastError());
    std::vector<int> slots(S, -1), loc_slots(S, -1);                                    /* the mapping lanes' frame, the localising lanes' */
    int n_map = 0, n_loc = 0;
    for (int q = 0; q < S; ++q) {
        if (cmd[q] == LL_DRIVE_IDLE) continue;
        if (d->map_of[q] >= 0) { loc_slots[q] = first + q; ++n_loc; continue; }         /* START resets no map */
        slots[q] = first + q; ++n_map;
        if (cmd[q] == LL_DRIVE_START) { rc = ll_cubemaps_reset(d->cms, q); if (rc) { d->err = drv_lane_msg(llcms_err(d->cms)); return rc; } }
    }
    std::vector<ScanHdr> hdr(S);
    if (n_map > 0 && d->map_vote_from >= 0) {                                           /* the reference's gate, now_frame > 20 (:2057) */
        std::vector<int> on(S, 0);
        for (int q = 0; q < S; ++q)
            if (slots[q] >= 0) on[q] = (cmd[q] == LL_DRIVE_START ? 0 : d->fidx[q] + 1) > d->map_vote_from;
        rc = ll_cubemaps_set_vote(d->cms, on.data());
        if (rc) { d->err = "mapping vote: " + drv_lane_msg(llcms_err(d->cms)); return rc; }
    }
    if (n_map > 0) {
        rc = llcms_process_slots_dev(d->cms, slots.data(), mapped.data(), ran.data(), d->d_odom, odom.data(), (size_t)S * 7 * sizeof(double), hdr.data());
        if (rc) { d->err = "mapping: " + drv_lane_msg(llcms_err(d->cms)); return rc; }
    }
    if (n_loc > 0) {                                                                    /* the step's guard: no map read here was written above */
        rc = llcms_localize_slots_dev(d->cms, loc_slots.data(), d->map_of.data(), mapped.data(), ran.data(), d->fit.data(), d->info_on ? d->info.data() : nullptr,
                                      d->d_odom, odom.data(),
                                      (size_t)S * 7 * sizeof(double), hdr.data());
        if (rc) { d->err = "localising: " + drv_lane_msg(llcms_err(d->cms)); return rc; }
    }
    hipLaunchKernelGGL(k_drives_update, dim3(nb), dim3(64), 0, st, S, d_cmd, d->d_odom, d->d_m2o, (const double *)d_map_pose);
    DRV_HIP(hipGetLastError());
    for (int q = 0; q < S; ++q) {                                                       /* what a checkpoint of the lane will hold of this slot */
        if (cmd[q] == LL_DRIVE_IDLE) continue;
        const bool ok = hdr[q].status == 0;                                             /* an empty scan is a target without points (ll_targets) */
        DrvFeat &f = d->feat[q];
        f.n[0] = ok ? hdr[q].n_sharp : 0; f.n[1] = ok ? hdr[q].n_less_sharp : 0; f.n[2] = ok ? hdr[q].n_flat : 0; f.n[3] = ok ? hdr[q].n_less_flat : 0;
        f.strided = ok ? hdr[q].lf_strided : 0;
    }
    if (d->keep_registered) {
        std::vector<DrvReg> tab;
        for (int q = 0; q < S; ++q) {
            d->reg_n[q] = 0;
            if (cmd[q] == LL_DRIVE_IDLE || hdr[q].status != 0) continue;
            d->reg_n[q] = std::min(hdr[q].n, ctx->V.CS);
            tab.push_back({q, first + q});
        }
        if (!tab.empty()) {
            const DrvReg *d_tab = (const DrvReg *)llcms_stage(d->cms, tab.data(), tab.size() * sizeof(DrvReg));
            if (!d_tab) { d->err = llcms_err(d->cms); return LL_ERR_HIP; }
            const LLView &V = ctx->V;
            hipLaunchKernelGGL(k_drives_register, dim3((unsigned)((V.ring_cap + 255) / 256), (unsigned)V.R, (unsigned)tab.size()), dim3(256), 0, st,
                               V, d_tab, (const double *)d_map_pose, d->d_reg);
            DRV_HIP(hipGetLastError());
        }
    }
    return LL_OK;
}

extern "C" int ll_drives_step(ll_drives *d, const int *cmd, const double *pose0, double *odom_w7, double *mapped_w7, int *ran)
{
    if (!d) return LL_ERR_ARG;
    if (!cmd) { d->err = "no commands"; return LL_ERR_ARG; }
    const int S = d->S;
    int n_run = 0;
    for (int q = 0; q < S; ++q) {
        const int c = cmd[q];
        if (c < LL_DRIVE_IDLE || c > LL_DRIVE_START) { d->err = "lane " + std::to_string(q) + ": command " + std::to_string(c) + " is not IDLE, RUN or START"; return LL_ERR_ARG; }
        if (c == LL_DRIVE_RUN && !d->ran_prev[q]) { d->err = "lane " + std::to_string(q) + ": RUN, but the lane did not run on the previous step (IDLE or START only)"; return LL_ERR_ARG; }
        if (c == LL_DRIVE_START && pose0)
            for (int k = 0; k < 7; ++k)
                if (!std::isfinite(pose0[(size_t)q * 7 + k])) { d->err = "lane " + std::to_string(q) + ": non-finite pose0"; return LL_ERR_ARG; }
        n_run += c != LL_DRIVE_IDLE;
    }
    for (int q = 0; q < S; ++q) {                                                       /* no step writes a map that a running lane reads */
        const int m = d->map_of[q];
        if (cmd[q] == LL_DRIVE_IDLE || m < 0 || m == q) continue;
        if (d->map_of[m] < 0 && cmd[m] != LL_DRIVE_IDLE) {
            d->err = "lane " + std::to_string(q) + " localises against the map of lane " + std::to_string(m) + ", which this step would map into: one of the two must be IDLE";
            return LL_ERR_ARG;
        }
    }
    std::vector<int> capture(S, 0), frame_tag(S, 0);                                    /* the lanes this step captures: room for them, or the step does not run */
    if (d->kf) {
        int n_cap = 0;
        for (int q = 0; q < S; ++q) {
            if (cmd[q] == LL_DRIVE_IDLE) continue;
            frame_tag[q] = cmd[q] == LL_DRIVE_START ? 0 : d->fidx[q] + 1;
            capture[q] = frame_tag[q] % d->kf_every == 0;
            n_cap += capture[q];
        }
        const ll_cubemap *cm = llcms_map(d->cms, 0);
        if (n_cap > 0 && llkf_room(d->kf, n_cap, cm->cap_last)) { d->err = "the step has not run: " + std::string(ll_keyframes_last_error(d->kf)); return LL_ERR_CAPACITY; }
    }
    std::fill(d->fit.begin(), d->fit.end(), ll_localize_fit());
    std::fill(d->info.begin(), d->info.end(), ll_pose_info());
    const double nan = std::nan("");
    std::vector<double> odom((size_t)S * 7, nan), mapped((size_t)S * 7, nan), p0((size_t)S * 7, 0.0);
    std::vector<int> r(S, 0);
    int rc = LL_OK;
    if (n_run > 0) {
        if (hipSetDevice(d->ctx->device) != hipSuccess) { d->err = "hipSetDevice failed"; return LL_ERR_HIP; }
        for (int q = 0; q < S; ++q) {
            if (cmd[q] != LL_DRIVE_START) continue;
            if (pose0) std::memcpy(&p0[(size_t)q * 7], pose0 + (size_t)q * 7, 7 * sizeof(double));
            else p0[(size_t)q * 7 + 3] = 1.0;
        }
        const long long s0 = llcms_syncs(d->cms);
        rc = drv_run(d, cmd, p0, odom, mapped, r);
        d->syncs += llcms_syncs(d->cms) - s0;
        d->row ^= 1;
        if (rc) {                                                                       /* the step is lost: its lanes are stopped */
            for (int q = 0; q < S; ++q) { d->ran_prev[q] = 0; if (cmd[q] != LL_DRIVE_IDLE) d->reg_n[q] = 0; }
            std::fill(d->fit.begin(), d->fit.end(), ll_localize_fit());
            std::fill(d->info.begin(), d->info.end(), ll_pose_info());
            return rc;
        }
        ++d->frames;
        if (d->kf) {                                                                    /* one copy launch, no synchronisation: the stack clouds stay as they are until the lane's next frame */
            rc = ll_keyframes_add_cubemaps(d->kf, d->cms, capture.data(), mapped.data(), nullptr, frame_tag.data(), nullptr);
            if (rc) { d->err = "capture: " + std::string(ll_keyframes_last_error(d->kf)); return rc; }
        }
    }
    for (int q = 0; q < S; ++q) {
        d->ran_prev[q] = cmd[q] != LL_DRIVE_IDLE;
        if (cmd[q] == LL_DRIVE_START) d->fidx[q] = 0;
        else if (cmd[q] == LL_DRIVE_RUN) d->fidx[q] += 1;
        else {
            d->reg_n[q] = 0;
            for (int k = 0; k < 7; ++k) { odom[(size_t)q * 7 + k] = nan; mapped[(size_t)q * 7 + k] = nan; }
            r[q] = 0;
        }
    }
    if (odom_w7) std::memcpy(odom_w7, odom.data(), odom.size() * sizeof(double));
    if (mapped_w7) std::memcpy(mapped_w7, mapped.data(), mapped.size() * sizeof(double));
    if (ran) std::memcpy(ran, r.data(), r.size() * sizeof(int));
    return LL_OK;
}

extern "C" int ll_drives_set_localize(ll_drives *d, const int *map_of, const double *start_w7)
{
    if (!d) return LL_ERR_ARG;
    if (!map_of) { d->err = "no map_of"; return LL_ERR_ARG; }
    const int S = d->S;
    std::vector<double> start((size_t)S * 7, 0.0);
    for (int q = 0; q < S; ++q) {
        if (map_of[q] < -1 || map_of[q] >= S) { d->err = "lane " + std::to_string(q) + ": map_of = " + std::to_string(map_of[q]) + " is neither -1 nor a lane"; return LL_ERR_ARG; }
        start[(size_t)q * 7 + 3] = 1.0;
        if (map_of[q] < 0 || !start_w7) continue;                                       /* a mapping lane starts at the identity, as ever */
        for (int k = 0; k < 7; ++k) {
            if (!std::isfinite(start_w7[(size_t)q * 7 + k])) { d->err = "lane " + std::to_string(q) + ": non-finite start pose"; return LL_ERR_ARG; }
            start[(size_t)q * 7 + k] = start_w7[(size_t)q * 7 + k];
        }
    }
    DRV_HIP(hipSetDevice(d->ctx->device));
    DRV_HIP(hipMemcpyAsync(d->d_start, start.data(), start.size() * sizeof(double), hipMemcpyHostToDevice, d->ctx->stream));
    DRV_HIP(hipStreamSynchronize(d->ctx->stream));                                      /* `start` goes away */
    d->map_of.assign(map_of, map_of + S);
    return LL_OK;
}

extern "C" int ll_drives_set_keyframes(ll_drives *d, ll_keyframes *kf, int every)
{
    if (!d) return LL_ERR_ARG;
    if (kf && every < 1) { d->err = "keyframes: every must be >= 1"; return LL_ERR_ARG; }
    if (kf && kf->ctx != d->ctx) { d->err = "keyframes: the store belongs to another context"; return LL_ERR_ARG; }
    d->kf = kf; d->kf_every = kf ? every : 1;
    return LL_OK;
}

extern "C" int ll_drives_correct(ll_drives *d, const int *lanes, const double *C_w7)
{
    if (!d) return LL_ERR_ARG;
    if (!lanes || !C_w7) { d->err = "correct: lanes or C_w7 is NULL"; return LL_ERR_ARG; }
    const int S = d->S;
    static const double ident[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    std::vector<int> sel(S, 0);
    std::vector<double> C((size_t)S * 7, 0.0);
    int n_sel = 0;
    for (int q = 0; q < S; ++q) {
        if (lanes[q] != 0 && lanes[q] != 1) { d->err = "correct: lane " + std::to_string(q) + ": the selector must be 0 or 1"; return LL_ERR_ARG; }
        if (!lanes[q]) continue;
        const double *Cq = C_w7 + (size_t)q * 7;
        for (int k = 0; k < 7; ++k) if (!std::isfinite(Cq[k])) { d->err = "correct: lane " + std::to_string(q) + ": non-finite C"; return LL_ERR_ARG; }
        if (!d->ran_prev[q]) { d->err = "correct: lane " + std::to_string(q) + " has no drive (it neither ran on the previous step nor was restored)"; return LL_ERR_STATE; }
        if (std::equal(Cq, Cq + 7, ident)) continue;                                    /* the identity is not applied: every bit stays, a -0.0 included */
        sel[q] = 1; ++n_sel;
        std::copy(Cq, Cq + 7, C.begin() + (size_t)q * 7);
    }
    if (n_sel == 0) return LL_OK;
    DRV_HIP(hipSetDevice(d->ctx->device));
    llcms_begin(d->cms);
    const int *d_sel = (const int *)llcms_stage(d->cms, sel.data(), sel.size() * sizeof(int));
    const double *d_C = (const double *)llcms_stage(d->cms, C.data(), C.size() * sizeof(double));
    if (!d_sel || !d_C) { d->err = llcms_err(d->cms); return LL_ERR_HIP; }
    hipLaunchKernelGGL(k_drives_correct, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, d->ctx->stream, S, d_sel, d_C, d->d_m2o);
    DRV_HIP(hipGetLastError());
    DRV_HIP(hipStreamSynchronize(d->ctx->stream));                                      /* outside a step: not counted */
    return LL_OK;
}

extern "C" int ll_drives_fit(ll_drives *d, ll_localize_fit *fit)
{
    if (!d) return LL_ERR_ARG;
    if (!fit) { d->err = "no fit array"; return LL_ERR_ARG; }
    std::memcpy(fit, d->fit.data(), d->fit.size() * sizeof(ll_localize_fit));
    return LL_OK;
}

/* the information records of the localising lanes: off after create; not part of a checkpoint */
extern "C" int ll_drives_set_info(ll_drives *d, int on)
{
    if (!d) return LL_ERR_ARG;
    if (on != 0 && on != 1) { d->err = "set_info: on must be 0 or 1"; return LL_ERR_ARG; }
    d->info_on = on;
    if (!on) std::fill(d->info.begin(), d->info.end(), ll_pose_info());
    return LL_OK;
}

extern "C" int ll_drives_info(ll_drives *d, ll_pose_info *info)
{
    if (!d) return LL_ERR_ARG;
    if (!info) { d->err = "no info array"; return LL_ERR_ARG; }
    std::memcpy(info, d->info.data(), d->info.size() * sizeof(ll_pose_info));
    return LL_OK;
}

extern "C" int ll_drives_registered(ll_drives *d, int lane, ll_point *out, int cap, int *n)
{
    if (!d || !n) return LL_ERR_ARG;
    if (lane < 0 || lane >= d->S) { d->err = "lane out of range"; return LL_ERR_ARG; }
    if (!d->keep_registered) { d->err = "created with keep_registered = 0"; return LL_ERR_STATE; }
    const int cnt = d->reg_n[lane];
    *n = cnt;
    if (!out) return LL_OK;
    if (cap < cnt) { d->err = "registered cloud capacity too small"; return LL_ERR_CAPACITY; }
    if (cnt > 0 && ll_read_back(out, d->d_reg + (size_t)lane * d->ctx->V.CS, (size_t)cnt * sizeof(float4), d->ctx->stream)) { d->err = "read-back failed"; return LL_ERR_HIP; }
    return LL_OK;
}

/* ------------------------------------------------------------------ lane checkpoints
 * A lane's state between two steps: its cube map (centre, per-cube counts, the two pools' live points, the valid list of its
 * last frame), d_odom, d_m2o, fidx, and the previous row's slot -- the four feature clouds and the solved pose, the target and
 * the warm start of its next odometry frame.  Pool offsets are not part of it: nothing reads a pool except through (off, cnt).
 * The blob (INTEGRATION.md has the table): CkHeader, n CkRecord, per record the counts [2][4851] and the valid list [125]
 * (host bookkeeping), then from a 256-byte boundary per record the device payload in 16-byte points: the LL_MAP_ALL cloud, sharp,
 * less sharp, flat, less flat (contiguous), LL_CK_STATE_PTS points of state.  Little-endian, as the hosts this library runs on. */
#define LL_CK_MAGIC 0x4B434C4Cu                  /* "LLCK" */
#define LL_CK_VERSION 1u
struct CkHeader {
    uint32_t magic, version, header_bytes, record_bytes;
    uint64_t total_bytes;
    uint32_t n_records; int32_t n_scans, distortion, voxel_sort_ranks;
    float line_res, plane_res;
    int32_t need[4];                             /* the largest sharp / less sharp / flat / less flat cloud of any record */
};
struct CkRecord {
    uint64_t tab_offset, offset, bytes;          /* counts + valid list; the device payload and its size */
    int64_t n_pts[2];                            /* corner, surf points of the map */
    int32_t lane, fidx, cen[3], n_valid, n_feat[4], rsv[4];
};
static_assert(sizeof(CkHeader) == 64 && sizeof(CkRecord) == 96, "the blob's fixed layout");
#define CK_COUNTS_BYTES ((size_t)((2 * CM_N * 4 + 15) / 16 * 16))
#define CK_TAB_BYTES (CK_COUNTS_BYTES + 512)
#define CK_MAX_RECORDS 4096

struct CkView { CkHeader h; std::vector<CkRecord> rec; };

static long long ck_payload_points(const CkRecord &r)
{
    return r.n_pts[0] + r.n_pts[1] + (long long)r.n_feat[0] + r.n_feat[1] + r.n_feat[2] + r.n_feat[3] + LL_CK_STATE_PTS;
}

/* every refusal a blob can earn on its own (LL_ERR_ARG, err names the field) */
static int ck_parse(const void *blob, long long bytes, CkView &v, std::string &err)
{
    if (!blob || bytes < 0) { err = "checkpoint: no blob"; return LL_ERR_ARG; }
    const unsigned char *b = (const unsigned char *)blob;
    uint32_t w = 0;
    if (bytes < 4) { err = "checkpoint: truncated before magic"; return LL_ERR_ARG; }
    std::memcpy(&w, b, 4);
    if (w != LL_CK_MAGIC) { err = "checkpoint: magic is not LLCK"; return LL_ERR_ARG; }
    if (bytes < 8) { err = "checkpoint: truncated before version"; return LL_ERR_ARG; }
    std::memcpy(&w, b + 4, 4);
    if (w != LL_CK_VERSION) { err = "checkpoint: version " + std::to_string(w) + ", this library reads " + std::to_string(LL_CK_VERSION); return LL_ERR_ARG; }
    if ((size_t)bytes < sizeof(CkHeader)) { err = "checkpoint: truncated inside the header"; return LL_ERR_ARG; }
    std::memcpy(&v.h, b, sizeof(CkHeader));
    const CkHeader &h = v.h;
    if (h.header_bytes != sizeof(CkHeader) || h.record_bytes != sizeof(CkRecord)) { err = "checkpoint: header_bytes / record_bytes do not match version 1"; return LL_ERR_ARG; }
    if (h.total_bytes != (uint64_t)bytes) { err = "checkpoint: total_bytes = " + std::to_string(h.total_bytes) + ", bytes = " + std::to_string(bytes) + (h.total_bytes > (uint64_t)bytes ? " (truncated)" : ""); return LL_ERR_ARG; }
    if (h.n_records > CK_MAX_RECORDS) { err = "checkpoint: n_records out of range"; return LL_ERR_ARG; }
    const uint64_t tab0 = sizeof(CkHeader) + (uint64_t)h.n_records * sizeof(CkRecord);
    if (tab0 > h.total_bytes) { err = "checkpoint: the record table runs past the end"; return LL_ERR_ARG; }
    if (h.n_scans < 1 || h.n_scans > LL_MAX_RINGS || !(h.line_res > 0.0f) || !(h.plane_res > 0.0f)) { err = "checkpoint: n_scans / line_res / plane_res out of range"; return LL_ERR_ARG; }
    v.rec.resize(h.n_records);
    if (h.n_records) std::memcpy(v.rec.data(), b + sizeof(CkHeader), (size_t)h.n_records * sizeof(CkRecord));
    std::vector<int> counts(2 * CM_N);
    /* the regions in the order a save writes them, none overlapping another: header, records, every record's tables, every record's payload */
    uint64_t tab_end = tab0;
    for (uint32_t r = 0; r < h.n_records; ++r) {
        const CkRecord &R = v.rec[r];
        if (R.tab_offset < tab_end || R.tab_offset > h.total_bytes || h.total_bytes - R.tab_offset < CK_TAB_BYTES) { err = "checkpoint: record " + std::to_string(r) + ": tab_offset overlaps what lies before it or runs past the end"; return LL_ERR_ARG; }
        tab_end = R.tab_offset + CK_TAB_BYTES;
    }
    uint64_t pay_end = tab_end;
    for (uint32_t r = 0; r < h.n_records; ++r) {
        const CkRecord &R = v.rec[r];
        const std::string who = "checkpoint: record " + std::to_string(r) + ": ";
        if (R.offset < pay_end || (R.offset & 15) || R.offset > h.total_bytes || h.total_bytes - R.offset < R.bytes) { err = who + "offset / bytes overlap what lies before them or run past the end"; return LL_ERR_ARG; }
        pay_end = R.offset + R.bytes;
        for (int k = 0; k < 4; ++k) if (R.n_feat[k] < 0) { err = who + "negative feature count"; return LL_ERR_ARG; }
        if (R.n_pts[0] < 0 || R.n_pts[1] < 0 || R.n_pts[0] > (1 << 26) || R.n_pts[1] > (1 << 26)) { err = who + "n_pts out of range"; return LL_ERR_ARG; }
        if ((uint64_t)ck_payload_points(R) * 16 != R.bytes) { err = who + "bytes does not match the counts"; return LL_ERR_ARG; }
        if (R.fidx < 0 || R.n_valid < 0 || R.n_valid > 125) { err = who + "fidx / n_valid out of range"; return LL_ERR_ARG; }
        std::memcpy(counts.data(), b + R.tab_offset, counts.size() * sizeof(int));
        long long tot[2] = {0, 0};
        for (int wv = 0; wv < 2; ++wv)
            for (int c = 0; c < CM_N; ++c) { if (counts[(size_t)wv * CM_N + c] < 0) { err = who + "negative cube count"; return LL_ERR_ARG; } tot[wv] += counts[(size_t)wv * CM_N + c]; }
        if (tot[0] != R.n_pts[0] || tot[1] != R.n_pts[1]) { err = who + "the cube counts do not add up to n_pts"; return LL_ERR_ARG; }
    }
    return LL_OK;
}

extern "C" int ll_checkpoint_describe(const void *blob, long long bytes, ll_checkpoint_info *info)
{
    if (!info) return LL_ERR_ARG;
    CkView v; std::string err;
    const int rc = ck_parse(blob, bytes, v, err);
    if (rc) return rc;
    info->version = (int)v.h.version; info->n_records = (int)v.h.n_records; info->total_bytes = (long long)v.h.total_bytes;
    info->n_scans = v.h.n_scans; info->distortion = v.h.distortion; info->voxel_sort_ranks = v.h.voxel_sort_ranks;
    info->line_res = v.h.line_res; info->plane_res = v.h.plane_res;
    for (int k = 0; k < 4; ++k) info->need_features[k] = v.h.need[k];
    if (info->records)
        for (int r = 0; r < (int)v.h.n_records && r < info->cap_records; ++r) {
            const CkRecord &R = v.rec[r];
            ll_checkpoint_record &o = info->records[r];
            o.lane = R.lane; o.frame_index = R.fidx; o.n_corner = R.n_pts[0]; o.n_surf = R.n_pts[1];
            for (int k = 0; k < 4; ++k) o.n_features[k] = R.n_feat[k];
            o.offset = (long long)R.offset; o.bytes = (long long)R.bytes;
        }
    return LL_OK;
}

/* the blob of the selected lanes: header, records, and where the device payload starts; host bookkeeping only */
static int ck_plan(ll_drives *d, const int *lanes, CkHeader &h, std::vector<CkRecord> &rec, uint64_t *dev_off)
{
    if (!lanes) { d->err = "checkpoint: no lane selection"; return LL_ERR_ARG; }
    rec.clear();
    for (int q = 0; q < d->S; ++q) {
        if (lanes[q] != 0 && lanes[q] != 1) { d->err = "lane " + std::to_string(q) + ": the selection must be 0 or 1"; return LL_ERR_ARG; }
        if (!lanes[q]) continue;
        if (!d->ran_prev[q]) { d->err = "lane " + std::to_string(q) + ": nothing to save (the lane neither ran on the previous step nor was restored since)"; return LL_ERR_STATE; }
        const ll_cubemap *cm = llcms_map(d->cms, q);
        if (cm->broken) { d->err = "lane " + std::to_string(q) + ": its map is unusable"; return LL_ERR_STATE; }
        CkRecord R;
        std::memset(&R, 0, sizeof(R));
        for (int w = 0; w < 2; ++w) for (int c = 0; c < CM_N; ++c) R.n_pts[w] += cm->cnt[w][c];
        R.lane = q; R.fidx = d->fidx[q]; R.n_valid = cm->n_valid;
        for (int k = 0; k < 3; ++k) R.cen[k] = cm->cen[k];
        for (int k = 0; k < 4; ++k) R.n_feat[k] = d->feat[q].n[k];
        R.bytes = (uint64_t)ck_payload_points(R) * 16;
        rec.push_back(R);
    }
    std::memset(&h, 0, sizeof(h));
    h.magic = LL_CK_MAGIC; h.version = LL_CK_VERSION; h.header_bytes = sizeof(CkHeader); h.record_bytes = sizeof(CkRecord);
    h.n_records = (uint32_t)rec.size();
    h.n_scans = d->ctx->p.n_scans; h.distortion = d->ctx->p.distortion; h.voxel_sort_ranks = d->ctx->p.voxel_sort_ranks;
    const ll_cubemap *cm0 = llcms_map(d->cms, 0);
    h.line_res = cm0->leaf[0]; h.plane_res = cm0->leaf[1];
    uint64_t at = sizeof(CkHeader) + rec.size() * sizeof(CkRecord);
    for (CkRecord &R : rec) { R.tab_offset = at; at += CK_TAB_BYTES; for (int k = 0; k < 4; ++k) h.need[k] = std::max(h.need[k], R.n_feat[k]); }
    at = (at + 255) & ~(uint64_t)255;
    *dev_off = at;
    for (CkRecord &R : rec) { R.offset = at; at += R.bytes; }
    h.total_bytes = at;
    return LL_OK;
}

extern "C" long long ll_drives_save_size(ll_drives *d, const int *lanes)
{
    if (!d) return LL_ERR_ARG;
    CkHeader h; std::vector<CkRecord> rec; uint64_t dev_off = 0;
    const int rc = ck_plan(d, lanes, h, rec, &dev_off);
    return rc ? (long long)rc : (long long)h.total_bytes;
}

extern "C" int ll_drives_save(ll_drives *d, const int *lanes, void *blob, long long cap, long long *bytes)
{
    if (!d) return LL_ERR_ARG;
    CkHeader h; std::vector<CkRecord> rec; uint64_t dev_off = 0;
    int rc = ck_plan(d, lanes, h, rec, &dev_off); if (rc) return rc;
    if (bytes) *bytes = (long long)h.total_bytes;
    if (cap < 0 || (uint64_t)cap < h.total_bytes) { d->err = "checkpoint: " + std::to_string(h.total_bytes) + " bytes, room for " + std::to_string(cap); return LL_ERR_CAPACITY; }
    if (!blob) { d->err = "checkpoint: blob is NULL"; return LL_ERR_ARG; }
    ll_ctx *ctx = d->ctx;
    const LLView &V = ctx->V;
    const int S = d->S, prev = d->base + (d->row ^ 1) * S;
    /* the host part, and the tables of the one pack launch */
    std::vector<unsigned char> host((size_t)dev_off, 0);
    std::memcpy(host.data(), &h, sizeof(h));
    if (!rec.empty()) std::memcpy(host.data() + sizeof(h), rec.data(), rec.size() * sizeof(CkRecord));
    std::vector<LLExpSeg> segs;
    std::vector<LLCkRec> recs;
    LLTiler tiles{llx_tile()};
    auto seg = [&](const float4 *src, long long at, int cnt) { if (cnt > 0) segs.push_back({src, at, cnt, tiles.take(cnt)}); };
    for (const CkRecord &R : rec) {
        const int q = R.lane, slot = prev + q;
        const ll_cubemap *cm = llcms_map(d->cms, q);
        for (int w = 0; w < 2; ++w) std::memcpy(host.data() + R.tab_offset + (size_t)w * CM_N * sizeof(int), cm->cnt[w].data(), CM_N * sizeof(int));
        std::memcpy(host.data() + R.tab_offset + CK_COUNTS_BYTES, cm->valid, (size_t)cm->n_valid * sizeof(int));
        long long at = (long long)((R.offset - dev_off) / 16);
        at += llx_segments(cm, LL_MAP_ALL, at, &tiles, &segs);
        seg(V.sharp + (size_t)slot * V.cap_sharp, at, R.n_feat[0]); at += R.n_feat[0];
        seg(V.lsharp + (size_t)slot * V.cap_lsharp, at, R.n_feat[1]); at += R.n_feat[1];
        seg(V.flat + (size_t)slot * V.cap_flat, at, R.n_feat[2]); at += R.n_feat[2];
        LLCkRec C;
        std::memset(&C, 0, sizeof(C));
        const float4 *lflat = V.lflat + (size_t)slot * V.LFS;
        if (d->feat[q].strided) { C.lflat = lflat; C.lf_pre = V.lf_pre + (size_t)slot * (V.R + 1); C.dst_lflat = at; C.n_lflat = R.n_feat[3]; C.ring_cap = V.ring_cap; }
        else seg(lflat, at, R.n_feat[3]);
        at += R.n_feat[3];
        C.pose = V.pose + (size_t)slot * 7; C.odom = d->d_odom + (size_t)q * 7; C.m2o = d->d_m2o + (size_t)q * 7; C.fidx = d->d_fidx + q; C.dst_state = at; C.bad = d->d_ck_bad;
        recs.push_back(C);
    }
    if (!tiles.fits()) { d->err = "checkpoint: too many tiles for one launch"; return LL_ERR_CAPACITY; }
    DRV_HIP(hipSetDevice(ctx->device));
    const size_t n_pts = (size_t)((h.total_bytes - dev_off) / 16);
    const bool direct = llx_is_device(blob);
    if (direct && ((uintptr_t)blob & 15)) { d->err = "checkpoint: a device blob must be 16-byte aligned"; return LL_ERR_ARG; }
    float4 *dst = direct ? (float4 *)((unsigned char *)blob + dev_off) : nullptr;
    if (!direct && n_pts > 0) {
        std::string why;
        dst = llx_reserve(llcms_export_state(d->cms), n_pts, why);
        if (!dst) { d->err = "checkpoint: " + why; return LL_ERR_HIP; }
    }
    llcms_begin(d->cms);
    const LLExpSeg *d_segs = segs.empty() ? nullptr : (const LLExpSeg *)llcms_stage(d->cms, segs.data(), segs.size() * sizeof(LLExpSeg));
    const LLCkRec *d_recs = recs.empty() ? nullptr : (const LLCkRec *)llcms_stage(d->cms, recs.data(), recs.size() * sizeof(LLCkRec));
    if ((!segs.empty() && !d_segs) || (!recs.empty() && !d_recs)) { d->err = llcms_err(d->cms); return LL_ERR_HIP; }
    int *bad = (int *)ll_pinned_scratch(sizeof(int));
    if (!bad) { d->err = "no page-locked scratch"; return LL_ERR_HIP; }
    DRV_HIP(hipMemsetAsync(d->d_ck_bad, 0, sizeof(int), ctx->stream));
    rc = llx_pack(ctx, d_segs, segs.size(), tiles.next, d_recs, (int)recs.size(), V.R, tiles.per, dst, d->err); if (rc) return rc;
    DRV_HIP(hipMemcpyAsync(bad, d->d_ck_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (direct) { if (!llcms_stage_to(d->cms, host.data(), host.size(), blob)) { d->err = llcms_err(d->cms); return LL_ERR_HIP; } }
    else if (n_pts > 0) DRV_HIP(hipMemcpyAsync((unsigned char *)blob + dev_off, dst, n_pts * 16, hipMemcpyDeviceToHost, ctx->stream));
    rc = llcms_sync(d->cms);
    if (rc) { d->err = llcms_err(d->cms); return rc; }
    ++d->syncs;
    if (*bad && direct) { (void)hipMemsetAsync(blob, 0, sizeof(CkHeader), ctx->stream); (void)hipStreamSynchronize(ctx->stream); }   /* no header: no checkpoint */
    if (*bad) { d->err = "checkpoint: a lane's less-flat cloud does not add up to the size in its scan header: nothing valid was written"; return LL_ERR_STATE; }
    if (!direct) std::memcpy(blob, host.data(), host.size());
    return LL_OK;
}

extern "C" int ll_drives_restore(ll_drives *d, const int *into, const void *blob, long long bytes)
{
    if (!d) return LL_ERR_ARG;
    if (!into) { d->err = "checkpoint: no lane mapping"; return LL_ERR_ARG; }
    if (blob && llx_is_device(blob)) { d->err = "checkpoint: restore reads the blob from host memory"; return LL_ERR_ARG; }
    CkView v;
    int rc = ck_parse(blob, bytes, v, d->err); if (rc) return rc;
    ll_ctx *ctx = d->ctx;
    LLView &V = ctx->V;
    const CkHeader &h = v.h;
    const ll_cubemap *cm0 = llcms_map(d->cms, 0);
    if (h.n_scans != ctx->p.n_scans) { d->err = "checkpoint: n_scans = " + std::to_string(h.n_scans) + ", the context has " + std::to_string(ctx->p.n_scans); return LL_ERR_ARG; }
    if (h.distortion != ctx->p.distortion) { d->err = "checkpoint: distortion = " + std::to_string(h.distortion) + ", the context has " + std::to_string(ctx->p.distortion); return LL_ERR_ARG; }
    if (h.line_res != cm0->leaf[0] || h.plane_res != cm0->leaf[1]) { d->err = "checkpoint: line_res / plane_res differ from the destination's"; return LL_ERR_ARG; }
    const int S = d->S, prev = d->base + (d->row ^ 1) * S;
    const unsigned char *b = (const unsigned char *)blob;
    std::vector<char> taken(S, 0);
    std::vector<std::vector<int>> tabs(v.rec.size());
    uint64_t lo = ~(uint64_t)0, hi = 0;
    const int cap_feat[4] = {V.cap_sharp, V.cap_lsharp, V.cap_flat, V.NP};
    const char *feat_name[4] = {"sharp", "less sharp", "flat", "less flat"};
    for (size_t r = 0; r < v.rec.size(); ++r) {
        const int q = into[r];
        if (q == -1) continue;
        const CkRecord &R = v.rec[r];
        if (q < 0 || q >= S) { d->err = "checkpoint: into[" + std::to_string(r) + "] = " + std::to_string(q) + " is no lane"; return LL_ERR_ARG; }
        if (taken[q]) { d->err = "checkpoint: two records go into lane " + std::to_string(q); return LL_ERR_ARG; }
        taken[q] = 1;
        tabs[r].assign(2 * CM_N + 125, 0);
        std::memcpy(tabs[r].data(), b + R.tab_offset, 2 * CM_N * sizeof(int));
        std::memcpy(tabs[r].data() + 2 * CM_N, b + R.tab_offset + CK_COUNTS_BYTES, 125 * sizeof(int));
        std::string why;
        rc = llx_import_check(llcms_map(d->cms, q), R.cen, tabs[r].data(), tabs[r].data() + 2 * CM_N, R.n_valid, R.n_pts[0] + R.n_pts[1], why);
        if (rc) { d->err = "checkpoint: record " + std::to_string(r) + " into lane " + std::to_string(q) + ": " + why; return rc; }
        for (int k = 0; k < 4; ++k)
            if (R.n_feat[k] > cap_feat[k]) { d->err = "checkpoint: record " + std::to_string(r) + ": " + std::to_string(R.n_feat[k]) + " " + feat_name[k] + " points, the context holds " + std::to_string(cap_feat[k]) + " per scan"; return LL_ERR_CAPACITY; }
        lo = std::min(lo, R.offset); hi = std::max(hi, R.offset + R.bytes);
    }
    if (hi <= lo) return LL_OK;                                                         /* every record skipped */
    std::vector<LLImpSeg> segs;
    std::vector<DrvRestore> tab;
    LLTiler tiles{llx_tile()};
    auto seg = [&](float4 *dst, long long at, int cnt) { if (cnt > 0) segs.push_back({dst, at, cnt, tiles.take(cnt)}); };
    for (size_t r = 0; r < v.rec.size(); ++r) {
        const int q = into[r];
        if (q < 0) continue;
        const CkRecord &R = v.rec[r];
        const int slot = prev + q;
        long long at = (long long)((R.offset - lo) / 16);
        llx_import_segments(llcms_map(d->cms, q), tabs[r].data(), at, tiles, &segs);
        at += R.n_pts[0] + R.n_pts[1];
        seg(V.sharp + (size_t)slot * V.cap_sharp, at, R.n_feat[0]); at += R.n_feat[0];
        seg(V.lsharp + (size_t)slot * V.cap_lsharp, at, R.n_feat[1]); at += R.n_feat[1];
        seg(V.flat + (size_t)slot * V.cap_flat, at, R.n_feat[2]); at += R.n_feat[2];
        seg(V.lflat + (size_t)slot * V.LFS, at, R.n_feat[3]); at += R.n_feat[3];
        DrvRestore T;
        std::memset(&T, 0, sizeof(T));
        T.src_state = at; T.slot = slot; T.lane = q;
        T.hdr.first_kept = 0; T.hdr.last_kept = -1;                                     /* ll_upload_features' header */
        T.hdr.n_sharp = R.n_feat[0]; T.hdr.n_less_sharp = R.n_feat[1]; T.hdr.n_flat = R.n_feat[2]; T.hdr.n_less_flat = R.n_feat[3];
        tab.push_back(T);
    }
    if (!tiles.fits()) { d->err = "checkpoint: too many tiles for one launch"; return LL_ERR_CAPACITY; }
    DRV_HIP(hipSetDevice(ctx->device));
    const size_t n_up = (size_t)((hi - lo) / 16);
    std::string why;
    float4 *src = llx_reserve(llcms_export_state(d->cms), n_up, why);
    if (!src) { d->err = "checkpoint: " + why; return LL_ERR_HIP; }
    llcms_begin(d->cms);
    const LLImpSeg *d_segs = segs.empty() ? nullptr : (const LLImpSeg *)llcms_stage(d->cms, segs.data(), segs.size() * sizeof(LLImpSeg));
    const DrvRestore *d_tab = (const DrvRestore *)llcms_stage(d->cms, tab.data(), tab.size() * sizeof(DrvRestore));
    if ((!segs.empty() && !d_segs) || !d_tab) { d->err = llcms_err(d->cms); return LL_ERR_HIP; }
    /* ---- from here on a failure loses the lanes being restored ---- */
    for (const DrvRestore &T : tab) { llcms_map(d->cms, T.lane)->broken = true; d->ran_prev[T.lane] = 0; d->reg_n[T.lane] = 0; }
    rc = llx_scatter(ctx, d_segs, segs.size(), tiles.next, src, b + lo, n_up, tiles.per, d->err); if (rc) return rc;
    hipLaunchKernelGGL(k_drives_restore, dim3((unsigned)tab.size()), dim3(64), 0, ctx->stream, d_tab, (const float4 *)src, V.pose, d->d_odom, d->d_m2o, d->d_fidx, V.hdr);
    for (size_t a = 0; a < tab.size();) {                                               /* the slots serve as targets: their search grids, one launch per run of neighbouring lanes */
        size_t e = a + 1;                                                               /* (tab is in record order: a save lists the lanes ascending) */
        while (e < tab.size() && tab[e].slot == tab[e - 1].slot + 1) ++e;
        ll_launch_build_grid(V, tab[a].slot, (int)(e - a), 0, ctx->stream, nullptr);
        a = e;
    }
    DRV_HIP(hipGetLastError());
    rc = llcms_sync(d->cms);
    if (rc) { d->err = llcms_err(d->cms); return rc; }
    ++d->syncs;
    for (size_t r = 0; r < v.rec.size(); ++r) {
        const int q = into[r];
        if (q < 0) continue;
        const CkRecord &R = v.rec[r];
        llx_import_commit(llcms_map(d->cms, q), R.cen, tabs[r].data(), tabs[r].data() + 2 * CM_N, R.n_valid);
        d->ran_prev[q] = 1; d->fidx[q] = R.fidx;
        for (int k = 0; k < 4; ++k) d->feat[q].n[k] = R.n_feat[k];
        d->feat[q].strided = 0;
        if ((size_t)(prev + q) < ctx->n_in_host.size()) ctx->n_in_host[prev + q] = 0;
        ctx->deskewed[prev + q] = ctx->deskew_mode != 0;                                 /* a saved carry holds the clouds as they were, and the slot is only ever a target */
    }
    return LL_OK;
}
