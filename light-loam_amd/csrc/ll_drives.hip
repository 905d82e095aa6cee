/*
 * ll_drives.hip -- whole drives side by side: S lanes, each running one drive at a time through registration, odometry and
 * mapping -- the chain of ll_odometry_kitti with mapping = 1 (extract, ll_odometry_frames, WorldPose, LaserMapping's
 * transformAssociateToMap / process_slot / transformUpdate) for every lane in one set of launches per stage.
 * The lanes' pose state lives on the device, so a step adds no host synchronisation to those of its cube-map frame:
 *   ll_extract_batch over the row, ll_odometry_sequences (one row, RUN lanes), k_drives_associate (world pose, :830-831, and
 *   transformAssociateToMap, laserMapping.cpp:113-117, straight into the cube maps' pose array), the cube-map frame from those
 *   guesses (ll_cubemaps.hip: they come to the host with the slot headers it reads back anyway), k_drives_update
 *   (transformUpdate, :119-123) and, with keep_registered, k_drives_register (pointAssociateToMap of laserCloud, :125-133).
 * The pose arithmetic restates lightloam::WorldPose::compose and LaserMapping::qmul / qrot (lightloam_host.hpp) in their
 * operation order, in double; the library is built with -ffp-contract=off, so it is bit for bit the host's.  No fma(), no
 * reassociation here.
 */
#include "ll_cubemap.h"
#include <cmath>

/* q (x, y, z, w) * v, LaserMapping::qrot */
__device__ __forceinline__ void drv_qrot(const double *q, const double *v, double *o)
{
    const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
    double uvx = uy * v[2] - uz * v[1], uvy = uz * v[0] - ux * v[2], uvz = ux * v[1] - uy * v[0];
    uvx += uvx; uvy += uvy; uvz += uvz;
    o[0] = v[0] + w * uvx + (uy * uvz - uz * uvy); o[1] = v[1] + w * uvy + (uz * uvx - ux * uvz); o[2] = v[2] + w * uvz + (ux * uvy - uy * uvx);
}

/* a * b, LaserMapping::qmul */
__device__ __forceinline__ void drv_qmul(const double *a, const double *b, double *o)
{
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    o[0] = aw * bx + ax * bw + ay * bz - az * by; o[1] = aw * by - ax * bz + ay * bw + az * bx;
    o[2] = aw * bz + ax * by - ay * bx + az * bw; o[3] = aw * bw - ax * bx - ay * by - az * bz;
}

/* per lane: odom [S][7] = q_w_curr, t_w_curr (laserOdometry); m2o [S][7] = q_wmap_wodom, t_wmap_wodom (laserMapping) */
__global__ __launch_bounds__(64) void k_drives_associate(double *vpose, int first, int S, const int *cmd, const double *pose0, double *odom,
                                                          double *m2o, int *fidx, double *map_pose)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= S) return;
    const int c = cmd[q];
    if (c == LL_DRIVE_IDLE) return;
    double *W = odom + (size_t)q * 7, *M = m2o + (size_t)q * 7, *slot_pose = vpose + (size_t)(first + q) * 7;
    if (c == LL_DRIVE_START) {
        for (int k = 0; k < 7; ++k) { W[k] = k == 3 ? 1.0 : 0.0; M[k] = k == 3 ? 1.0 : 0.0; }
        for (int k = 0; k < 7; ++k) slot_pose[k] = pose0[(size_t)q * 7 + k];     /* the warm start of frame 1 (:61-65) */
        fidx[q] = 0;
    } else {                                                                      /* WorldPose::compose (:830-831) */
        const double ql[4] = {slot_pose[0], slot_pose[1], slot_pose[2], slot_pose[3]}, tl[3] = {slot_pose[4], slot_pose[5], slot_pose[6]};
        const double ux = W[0], uy = W[1], uz = W[2], w = W[3];
        double uv[3] = {uy * tl[2] - uz * tl[1], uz * tl[0] - ux * tl[2], ux * tl[1] - uy * tl[0]};
        for (int k = 0; k < 3; ++k) uv[k] += uv[k];
        W[4] += (tl[0] + w * uv[0]) + (uy * uv[2] - uz * uv[1]);
        W[5] += (tl[1] + w * uv[1]) + (uz * uv[0] - ux * uv[2]);
        W[6] += (tl[2] + w * uv[2]) + (ux * uv[1] - uy * uv[0]);
        const double ax = W[0], ay = W[1], az = W[2], aw = W[3], bx = ql[0], by = ql[1], bz = ql[2], bw = ql[3];
        W[3] = aw * bw - ax * bx - ay * by - az * bz;
        W[0] = aw * bx + ax * bw + ay * bz - az * by;
        W[1] = aw * by - ax * bz + ay * bw + az * bx;
        W[2] = aw * bz + ax * by - ay * bx + az * bw;
        fidx[q] += 1;
    }
    double P[7], r[3];                                                            /* transformAssociateToMap (:113-117) */
    drv_qmul(M, W, P);
    drv_qrot(M, W + 4, r);
    for (int k = 0; k < 3; ++k) P[4 + k] = r[k] + M[4 + k];
    for (int k = 0; k < 7; ++k) map_pose[(size_t)q * 7 + k] = P[k];
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
    drv_qmul(P, inv, qm);
    drv_qrot(qm, tc, r);
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
    const double *pose = map_pose + (size_t)L.lane * 7;
    const double ux = pose[0], uy = pose[1], uz = pose[2], w = pose[3];
    const double v[3] = {(double)p.x, (double)p.y, (double)p.z};
    double uvx = uy * v[2] - uz * v[1], uvy = uz * v[0] - ux * v[2], uvz = ux * v[1] - uy * v[0];
    uvx += uvx; uvy += uvy; uvz += uvz;
    const float sx = (float)(((v[0] + w * uvx) + (uy * uvz - uz * uvy)) + pose[4]);
    const float sy = (float)(((v[1] + w * uvy) + (uz * uvx - ux * uvz)) + pose[5]);
    const float sz = (float)(((v[2] + w * uvz) + (ux * uvy - uy * uvx)) + pose[6]);
    out[(size_t)L.lane * V.CS + off + i] = make_float4(sx, sy, sz, p.w);
}

/* ------------------------------------------------------------------ host side */
struct ll_drives {
    ll_ctx *ctx = nullptr;
    ll_cubemaps *cms = nullptr;
    int S = 0, base = 0, n_outer = 3, keep_registered = 0;
    int row = 0;                                  /* the row the next step reads */
    std::vector<int> ran_prev, fidx, reg_n;       /* per lane: ran on the last step, frame index of its last frame, registered points */
    double *d_odom = nullptr, *d_m2o = nullptr;   /* [S][7] each */
    int *d_fidx = nullptr;                        /* [S]: the frame counter, mirrored on the device */
    float4 *d_reg = nullptr;                      /* [S][CS] registered clouds (keep_registered) */
    std::vector<void *> allocs;
    long long syncs = 0, frames = 0;
    std::string err;
};

#define DRV_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) { d->err = std::string(#call) + ": " + hipGetErrorString(e_); return LL_ERR_HIP; } \
    } while (0)

template <typename T>
static bool drv_alloc(ll_drives *d, T *&ptr, size_t count)
{
    void *p = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    if (hipMalloc(&p, bytes) != hipSuccess) { d->err = "hipMalloc failed (" + std::to_string(bytes) + " bytes)"; return false; }
    d->allocs.push_back(p);
    if (hipMemset(p, 0, bytes) != hipSuccess) { d->err = "hipMemset failed"; return false; }
    ptr = (T *)p;
    return true;
}

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
    d->ran_prev.assign(S, 0); d->fidx.assign(S, 0); d->reg_n.assign(S, 0);
    bool ok = drv_alloc(d, d->d_odom, (size_t)S * 7) && drv_alloc(d, d->d_m2o, (size_t)S * 7) && drv_alloc(d, d->d_fidx, (size_t)S);
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
    hipLaunchKernelGGL(k_drives_associate, dim3(nb), dim3(64), 0, st, ctx->V.pose, first, S, d_cmd, d_p0, d->d_odom, d->d_m2o, d->d_fidx, d_map_pose);
    DRV_HIP(hipGetLastError());
    std::vector<int> slots(S, -1);
    for (int q = 0; q < S; ++q) {
        if (cmd[q] == LL_DRIVE_IDLE) continue;
        slots[q] = first + q;
        if (cmd[q] == LL_DRIVE_START) { rc = ll_cubemaps_reset(d->cms, q); if (rc) { d->err = drv_lane_msg(llcms_err(d->cms)); return rc; } }
    }
    std::vector<ScanHdr> hdr(S);
    rc = llcms_process_slots_dev(d->cms, slots.data(), mapped.data(), ran.data(), d->d_odom, odom.data(), (size_t)S * 7 * sizeof(double), hdr.data());
    if (rc) { d->err = "mapping: " + drv_lane_msg(llcms_err(d->cms)); return rc; }
    hipLaunchKernelGGL(k_drives_update, dim3(nb), dim3(64), 0, st, S, d_cmd, d->d_odom, d->d_m2o, (const double *)d_map_pose);
    DRV_HIP(hipGetLastError());
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
            return rc;
        }
        ++d->frames;
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
