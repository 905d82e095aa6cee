/*
 * ll_visibility.hip -- ll_visibility: which stored keyframe points did OTHER frames of the same drive look straight through?  The
 * range-image visibility test of Removert (Kim & Kim, IROS 2020) and Pomerleau et al. (ICRA 2014) over the clouds of an
 * ll_keyframes store; not in the reference, the contract is in include/lightloam_hip.h.  ll_cubemaps_insert_keyframes_filtered
 * (ll_map_merge.hip) leaves the points out that a rule over the two counters removes.
 *
 * Every listed frame of a call has a list position k (counted across the ops); the host knows every size from the store's table
 * and builds ONE table blob: the (position, type) clouds where they lie in the pool with their first tiles, the poses [L][7], the
 * observer lists as CSR over list positions.
 *   k_vis_image   a workgroup takes one 1024-point tile of one (frame, type) cloud (segment table and binary search as k_kf_assign):
 *                 range, column and row per point in f32, an integer atomic minimum on the range's bits into raw[k] -- ranges are
 *                 positive, so the unsigned order is the floats', and a minimum does not depend on the order of arrival;
 *   k_vis_erode   one thread per pixel of every listed frame: img = the minimum of raw over the 3 x 3 pixels around it, columns wrap;
 *   k_vis_vote    a workgroup takes one tile of a subject cloud: the points are loaded once and taken to the world once
 *                 (ll_map_to_world), then the loop over the subject frame's observers -- pose and image base are the same for every
 *                 lane and come through uniform loads --: the inverse transform in f64, the pixel arithmetic, ONE image read, two
 *                 integer counts in registers; stored once as two bytes per point at the point's pool index.
 * No floating-point atomic, no sum whose order could matter: a frame's counters are the same bits alone, in any batch, in any order.
 * ll_visibility_run enqueues one table upload, one fill of raw and the three launches, and synchronises ONCE (the page-locked table
 * is free again, the events can be read).
 */
#include "ll_keyframes.h"
#include "ll_map_export.h"
#include "ll_map_search.h"
#include "ll_tiles.h"
#include <cmath>

#define VIS_TILE 1024
#define VIS_TWO_PI 6.2831855f
#define VIS_INF_BITS 0x7f800000u

struct VisCfg { int W, H; float el_min, ka, ke, rmin, rmax, mabs, mrel; };
struct VisSeg { long long off; int cnt; unsigned tile0; int k, pad; };    /* off: the cloud's first point in the pool; k: list position */

/* the pixel (row * W + col) of a point in a frame's sensor frame and its range; -1: no pixel (outside the range or elevation window, NaN) */
__device__ __forceinline__ int vis_pixel(float x, float y, float z, const VisCfg &c, float &r)
{
    const float xy2 = x * x + y * y;
    r = sqrtf(xy2 + z * z);
    if (!(r >= c.rmin && r < c.rmax)) return -1;                    /* also a NaN; what passes is finite */
    float a = ll_atan2f_finite(y, x);                              /* == ll_atan2f for finite operands (tests/test_exact_math.py) */
    if (a < 0.0f) a += VIS_TWO_PI;
    const int col = min(c.W - 1, (int)(a * c.ka));
    const float e = ll_atan2f_finite(z, sqrtf(xy2));
    const float fr = floorf((e - c.el_min) * c.ke);
    if (!(fr >= 0.0f && fr < (float)c.H)) return -1;
    return (int)fr * c.W + col;
}

__global__ __launch_bounds__(256) void k_vis_image(const float4 *__restrict__ pool, const VisSeg *__restrict__ seg, int nseg, VisCfg c, unsigned *raw)
{
    const VisSeg s = seg[ll_tile_find(seg, nseg, blockIdx.x)];
    const int first = (int)(blockIdx.x - s.tile0) * VIS_TILE, n = min(VIS_TILE, s.cnt - first);
    const float4 *src = pool + s.off + first;
    unsigned *im = raw + (size_t)s.k * ((size_t)c.W * c.H);
    float4 po[VIS_TILE / 256];
#pragma unroll
    for (int k = 0; k < VIS_TILE / 256; ++k) po[k] = src[min(k * 256 + (int)threadIdx.x, n - 1)];
#pragma unroll
    for (int k = 0; k < VIS_TILE / 256; ++k) {
        if (k * 256 + (int)threadIdx.x >= n) continue;
        float r;
        const int pix = vis_pixel(po[k].x, po[k].y, po[k].z, c, r);
        if (pix >= 0) atomicMin(&im[pix], __float_as_uint(r));
    }
}

/* grid (listed frames, pixel blocks) */
__global__ __launch_bounds__(256) void k_vis_erode(const unsigned *__restrict__ raw, unsigned *__restrict__ img, int W, int H)
{
    const int pix = blockIdx.y * 256 + (int)threadIdx.x;
    if (pix >= W * H) return;
    const size_t base = (size_t)blockIdx.x * ((size_t)W * H);
    const int row = pix / W, col = pix - row * W;
    const int cl = col == 0 ? W - 1 : col - 1, cr = col == W - 1 ? 0 : col + 1;
    unsigned m = VIS_INF_BITS;
#pragma unroll
    for (int dr = -1; dr <= 1; ++dr) {
        const int rr = row + dr;
        if (rr < 0 || rr >= H) continue;
        const unsigned *line = raw + base + (size_t)rr * W;
        m = min(m, min(line[cl], min(line[col], line[cr])));
    }
    img[base + pix] = m;
}

__global__ __launch_bounds__(256) void k_vis_vote(const float4 *__restrict__ pool, const VisSeg *__restrict__ seg, int nseg, const double *__restrict__ poses,
                                                  const int *__restrict__ obs_start, const int *__restrict__ obs, VisCfg c, const float *__restrict__ img,
                                                  unsigned char *cnt)
{
    const VisSeg s = seg[ll_tile_find(seg, nseg, blockIdx.x)];
    const int first = (int)(blockIdx.x - s.tile0) * VIS_TILE, n = min(VIS_TILE, s.cnt - first);
    const float4 *src = pool + s.off + first;
    const int ka = __builtin_amdgcn_readfirstlane(s.k);
    float wx[VIS_TILE / 256], wy[VIS_TILE / 256], wz[VIS_TILE / 256];
    int through[VIS_TILE / 256], hit[VIS_TILE / 256];
    {
        double PA[7];
        for (int k = 0; k < 7; ++k) PA[k] = poses[(size_t)ka * 7 + k];
        float4 po[VIS_TILE / 256];
#pragma unroll
        for (int k = 0; k < VIS_TILE / 256; ++k) po[k] = src[min(k * 256 + (int)threadIdx.x, n - 1)];
#pragma unroll
        for (int k = 0; k < VIS_TILE / 256; ++k) { ll_map_to_world(PA, po[k], wx[k], wy[k], wz[k]); through[k] = 0; hit[k] = 0; }
    }
    const int o0 = __builtin_amdgcn_readfirstlane(obs_start[ka]), o1 = __builtin_amdgcn_readfirstlane(obs_start[ka + 1]);
    const size_t HW = (size_t)c.W * c.H;
    for (int o = o0; o < o1; ++o) {
        const int b = __builtin_amdgcn_readfirstlane(obs[o]);
        double PB[7];
        for (int k = 0; k < 7; ++k) PB[k] = poses[(size_t)b * 7 + k];
        const float *im = img + (size_t)b * HW;
#pragma unroll
        for (int k = 0; k < VIS_TILE / 256; ++k) {
            float lx, ly, lz, r;
            vis_world_to_frame(PB, wx[k], wy[k], wz[k], lx, ly, lz);
            const int pix = vis_pixel(lx, ly, lz, c, r);
            if (pix < 0) continue;
            const float d = im[pix];
            const float m = c.mabs + c.mrel * r;
            const float r_far = r + m, r_near = r - m;
            if (d == __uint_as_float(VIS_INF_BITS)) continue;      /* B saw nothing there */
            if (d > r_far) ++through[k];
            else if (d >= r_near) ++hit[k];
        }
    }
    uchar2 *out = (uchar2 *)cnt + s.off + first;
#pragma unroll
    for (int k = 0; k < VIS_TILE / 256; ++k) {
        const int i = k * 256 + (int)threadIdx.x;
        if (i < n) out[i] = make_uchar2((unsigned char)min(through[k], 255), (unsigned char)min(hit[k], 255));
    }
}

/* ------------------------------------------------------------------ host side */
#define VIS_HIP(call) LL_HIP_CHECK(ll_fail, v, "visibility: ", call, #call)
#define VIS_RESET_SINCE "the store was reset since the counters were made: call ll_visibility_reset"

extern "C" void ll_visibility_default_params(ll_visibility_params *p)
{
    if (!p) return;
    p->width = 360; p->height = 90; p->el_min_deg = -45.0f; p->el_max_deg = 45.0f; p->min_range = 1.0f; p->max_range = 120.0f;
    p->margin_abs = 0.5f; p->margin_rel = 0.02f; p->radius = 40.0f; p->max_images = 256;
}

static VisCfg vis_cfg(const ll_visibility_params &p)
{
    const double rad = M_PI / 180.0;
    VisCfg c;
    c.W = p.width; c.H = p.height;
    c.el_min = (float)((double)p.el_min_deg * rad);
    c.ka = (float)((double)p.width / (2.0 * M_PI));
    c.ke = (float)((double)p.height / (((double)p.el_max_deg - (double)p.el_min_deg) * rad));
    c.rmin = p.min_range; c.rmax = p.max_range; c.mabs = p.margin_abs; c.mrel = p.margin_rel;
    return c;
}

extern "C" int ll_visibility_create(ll_keyframes *kf, const ll_visibility_params *p, ll_visibility **out)
{
    if (!kf || !p || !out) return LL_ERR_ARG;
    *out = nullptr;
    if (p->width < 8 || p->width > 4096 || p->height < 2 || p->height > 1024 || !(p->el_min_deg < p->el_max_deg) || !(p->el_min_deg >= -89.0f) ||
        !(p->el_max_deg <= 89.0f) || p->max_images < 2 || p->max_images > (1 << 16) || !(p->min_range >= 0.0f) || !(p->max_range > p->min_range) ||
        !std::isfinite(p->max_range) || !(p->margin_abs >= 0.0f) || !(p->margin_rel >= 0.0f) || !std::isfinite(p->margin_abs) ||
        !std::isfinite(p->margin_rel) || !(p->radius >= 0.0f) || !std::isfinite(p->radius))
        return llkf_create_err(kf, LL_ERR_ARG, "visibility: bad parameters (width in 8 .. 4096, height in 2 .. 1024, -89 <= el_min_deg < el_max_deg <= 89, "
                                          "max_images in 2 .. 2^16, 0 <= min_range < max_range, margins and radius finite and >= 0)");
    ll_ctx *ctx = kf->ctx;
    if (hipSetDevice(ctx->device) != hipSuccess) return llkf_create_err(kf, LL_ERR_HIP, "visibility: hipSetDevice failed");
    ll_visibility *v = new ll_visibility();
    v->follow(kf); v->p = *p;
    const size_t n_cnt = (size_t)(kf->cap[0] + kf->cap[1]) * 2, n_pix = (size_t)p->max_images * p->width * p->height;
    bool ok = hipMalloc((void **)&v->d_cnt, n_cnt) == hipSuccess && hipMalloc((void **)&v->d_raw, n_pix * 4) == hipSuccess &&
              hipMalloc((void **)&v->d_img, n_pix * 4) == hipSuccess;
    for (int k = 0; ok && k < 4; ++k) ok = hipEventCreate(&v->ev[k]) == hipSuccess;
    ok = ok && hipMemsetAsync(v->d_cnt, 0, n_cnt, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ll_visibility_destroy(v);
        return llkf_create_err(kf, LL_ERR_HIP, "visibility: no device memory for " + std::to_string(n_cnt) + " counter bytes and 2 x " + std::to_string(n_pix) + " pixels");
    }
    *out = v;
    return LL_OK;
}

extern "C" void ll_visibility_destroy(ll_visibility *v)
{
    if (!v) return;
    v->release();
    if (v->d_cnt) (void)hipFree(v->d_cnt);
    if (v->d_raw) (void)hipFree(v->d_raw);
    if (v->d_img) (void)hipFree(v->d_img);
    for (int k = 0; k < 4; ++k) if (v->ev[k]) (void)hipEventDestroy(v->ev[k]);
    delete v;
}

extern "C" const char *ll_visibility_last_error(const ll_visibility *v) { return v ? v->err.c_str() : "null visibility"; }

static int vis_stale(ll_visibility *v) { return v->stale("visibility: " VIS_RESET_SINCE); }

extern "C" int ll_visibility_reset(ll_visibility *v)
{
    if (!v) return LL_ERR_ARG;
    VIS_HIP(hipSetDevice(v->ctx->device));
    VIS_HIP(hipMemsetAsync(v->d_cnt, 0, (size_t)(v->kf->cap[0] + v->kf->cap[1]) * 2, v->ctx->stream));
    v->epoch = v->kf->n_reset; v->last.clear();
    for (int k = 0; k < 3; ++k) { v->ms[k] = 0.0; v->counts[k] = 0; }
    return LL_OK;
}

extern "C" int ll_visibility_run(ll_visibility *v, const ll_visibility_op *ops, int n_ops, long long *pairs)
{
    if (!v) return LL_ERR_ARG;
    if (!ops || n_ops < 1) return v->fail(LL_ERR_ARG, "visibility: ops is NULL or n_ops < 1");
    const ll_keyframes *kf = v->kf;
    const ll_keyframe_info *tab = kf->tab.data();
    const int size = (int)kf->tab.size();
    /* ---- every refusal before anything is enqueued or a counter changes */
    long long L = 0;
    std::vector<int> seen(size, -1);
    for (int i = 0; i < n_ops; ++i) {
        const ll_visibility_op &o = ops[i];
        const std::string who = "visibility: op " + std::to_string(i) + ": ";
        if (o.n_frames < 0 || (o.n_frames > 0 && !o.frames)) return v->fail(LL_ERR_ARG, who + "n_frames < 0 or frames is NULL");
        long long pts;
        if (llkf_check(tab, size, {o.n_frames, o.frames, o.poses_w7, ""}, LLKF_DUP_PER_CALL, &seen, i, who, &v->err, &pts)) return LL_ERR_ARG;
        L += o.n_frames;
    }
    if (L > (long long)v->p.max_images) return v->fail(LL_ERR_CAPACITY, "visibility: " + std::to_string(L) + " listed frames, max_images is " + std::to_string(v->p.max_images));
    int rc = vis_stale(v); if (rc) return rc;
    /* ---- the tables: clouds, poses, observers (CSR over list positions) */
    std::vector<VisSeg> segs;
    std::vector<double> poses((size_t)L * 7);
    std::vector<int> obs_start((size_t)L + 1, 0), obs, listed((size_t)L);
    LLTiler tiles{VIS_TILE};
    long long n_points = 0, n_pairs = 0;
    const double rad2 = (double)v->p.radius * (double)v->p.radius;
    int k0 = 0;
    for (int i = 0; i < n_ops; ++i) {
        const ll_visibility_op &o = ops[i];
        const LLKfList list = {o.n_frames, o.frames, o.poses_w7, ""};
        for (int f = 0; f < o.n_frames; ++f) {
            const double *P = llkf_pose(tab, list, f);
            for (int k = 0; k < 7; ++k) poses[(size_t)(k0 + f) * 7 + k] = P[k];
            listed[k0 + f] = o.frames[f];
            for (int w = 0; w < 2; ++w) {
                const LLKfCloud c = llkf_cloud(tab, kf->cap[0], o.frames[f], w);
                if (c.cnt <= 0) continue;
                segs.push_back({c.off, c.cnt, tiles.take(c.cnt), k0 + f, 0});
                n_points += c.cnt;
            }
        }
        long long np = 0;
        for (int a = 0; a < o.n_frames; ++a) {                     /* a frame does not observe itself: by position in the list */
            const double *A = &poses[(size_t)(k0 + a) * 7 + 4];
            for (int b = 0; b < o.n_frames; ++b) {
                if (b == a) continue;
                const double *B = &poses[(size_t)(k0 + b) * 7 + 4];
                const double dx = A[0] - B[0], dy = A[1] - B[1], dz = A[2] - B[2];
                if (dx * dx + dy * dy + dz * dz <= rad2) { obs.push_back(k0 + b); ++np; }
            }
            obs_start[k0 + a + 1] = (int)obs.size();
        }
        if (pairs) pairs[i] = np;
        n_pairs += np;
        k0 += o.n_frames;
    }
    if (!ll_grid_fits(obs.size()) || !tiles.fits()) return v->fail(LL_ERR_CAPACITY, "visibility: too many frame pairs or tiles for one call");
    v->last = listed;
    v->ms[0] = v->ms[1] = v->ms[2] = 0.0;
    v->counts[0] = L; v->counts[1] = n_points; v->counts[2] = n_pairs;
    if (L == 0) return LL_OK;
    if (obs.empty()) obs.push_back(0);                              /* never read: keeps the table's last part non-empty */
    std::vector<unsigned char> blob;
    const size_t at_seg = ll_blob_put(blob, segs), at_pose = ll_blob_put(blob, poses), at_start = ll_blob_put(blob, obs_start), at_obs = ll_blob_put(blob, obs);
    hipStream_t st = v->ctx->stream;
    VIS_HIP(hipSetDevice(v->ctx->device));
    const unsigned char *d_blob = (const unsigned char *)llx_stage_bytes(v->X, blob.data(), blob.size(), st, v->err);
    if (!d_blob) return LL_ERR_HIP;
    const VisCfg c = vis_cfg(v->p);
    const size_t HW = (size_t)c.W * c.H;
    const VisSeg *d_seg = (const VisSeg *)(d_blob + at_seg);
    VIS_HIP(hipMemsetD32Async((hipDeviceptr_t)v->d_raw, (int)VIS_INF_BITS, (size_t)L * HW, st));
    VIS_HIP(hipEventRecord(v->ev[0], st));
    if (tiles.next > 0) hipLaunchKernelGGL(k_vis_image, dim3((unsigned)tiles.next), dim3(256), 0, st, (const float4 *)kf->pool, d_seg, (int)segs.size(), c, (unsigned *)v->d_raw);
    VIS_HIP(hipEventRecord(v->ev[1], st));
    hipLaunchKernelGGL(k_vis_erode, dim3((unsigned)L, (unsigned)((HW + 255) / 256)), dim3(256), 0, st, (const unsigned *)v->d_raw, (unsigned *)v->d_img, c.W, c.H);
    VIS_HIP(hipEventRecord(v->ev[2], st));
    if (tiles.next > 0)
        hipLaunchKernelGGL(k_vis_vote, dim3((unsigned)tiles.next), dim3(256), 0, st, (const float4 *)kf->pool, d_seg, (int)segs.size(), (const double *)(d_blob + at_pose),
                           (const int *)(d_blob + at_start), (const int *)(d_blob + at_obs), c, (const float *)v->d_img, v->d_cnt);
    VIS_HIP(hipEventRecord(v->ev[3], st));
    VIS_HIP(hipGetLastError());
    VIS_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 3; ++k) v->ms[k] = ll_event_ms(v->ev[k], v->ev[k + 1], v->ms[k]);
    return LL_OK;
}

extern "C" int ll_visibility_counts(ll_visibility *v, int frame, unsigned char *through_hit)
{
    if (!v) return LL_ERR_ARG;
    if (!through_hit) return v->fail(LL_ERR_ARG, "visibility: through_hit is NULL");
    const ll_keyframes *kf = v->kf;
    long long pts;                                                  /* a list of one: the stored pose is finite, add refuses others */
    if (llkf_check(kf->tab.data(), (int)kf->tab.size(), {1, &frame, nullptr, ""}, LLKF_DUP_ALLOWED, nullptr, 0, "visibility: ", &v->err, &pts)) return LL_ERR_ARG;
    const int rc = vis_stale(v); if (rc) return rc;
    if (pts == 0) return LL_OK;
    const LLKfCloud c0 = llkf_cloud(kf->tab.data(), kf->cap[0], frame, 0), c1 = llkf_cloud(kf->tab.data(), kf->cap[0], frame, 1);
    const size_t n0 = (size_t)c0.cnt * 2, n1 = (size_t)c1.cnt * 2;
    const LLKfRange ranges[2] = {{v->d_cnt + (size_t)c0.off * 2, n0, through_hit}, {v->d_cnt + (size_t)c1.off * 2, n1, through_hit + n0}};
    return v->read("visibility: ", ranges, 2);
}

extern "C" int ll_visibility_images(ll_visibility *v, int k, float *raw, float *img)
{
    if (!v) return LL_ERR_ARG;
    if (k < 0 || k >= (int)v->last.size()) return v->fail(LL_ERR_ARG, "visibility: the last run listed " + std::to_string(v->last.size()) + " frames, there is no image " + std::to_string(k));
    const size_t HW = (size_t)v->p.width * v->p.height, bytes = HW * sizeof(float);
    if (!raw && !img) return LL_OK;
    const LLKfRange ranges[2] = {{raw ? v->d_raw + (size_t)k * HW : nullptr, bytes, raw}, {img ? v->d_img + (size_t)k * HW : nullptr, bytes, img}};
    return v->read("visibility: ", ranges, 2);
}

extern "C" int ll_visibility_timing(const ll_visibility *v, double *ms, long long *counts)
{
    return v ? llkf_timing(v->ms, v->counts, 3, ms, counts) : LL_ERR_ARG;
}

/* for the filtered insert (ll_map_merge.hip): is v usable with kf?  LL_OK, or the status with *why filled */
int llvis_check(const ll_visibility *v, const ll_keyframes *kf, std::string *why)
{
    if (v->kf != kf) { *why = "the visibility object belongs to another store"; return LL_ERR_ARG; }
    if (v->epoch != kf->n_reset) { *why = VIS_RESET_SINCE; return LL_ERR_STATE; }
    return LL_OK;
}
