/*
 * ll_bev.hip -- ll_bev: from a place match to a guess.  Correlative scan matching on bird's-eye occupancy grids (Olson, ICRA 2009;
 * the loop-closure matcher of Cartographer, Hess et al., ICRA 2016) over the clouds of an ll_keyframes store; not in the reference,
 * the contract -- the definition every number below follows -- is in include/lightloam_hip.h.
 *
 * The host knows every size from the store's table and builds ONE table blob: the listed (op, side, frame, type) clouds where they
 * lie in the pool with their first tiles, the poses, per op where its query list and its rows of the volume begin, per (op, yaw)
 * the cosine and sine.
 *   k_bev_prepare  a workgroup takes one 1024-point tile of one cloud (segment table and binary search as k_kf_assign): to the world
 *                  under the frame's pose, into the anchor's frame, cell and layer in f32.  A target tile ORs its bits into the op's
 *                  grid in HBM (a byte per cell, 32-bit integer atomic OR: order-free); a query tile writes (x, y) and the layer at
 *                  the point's own position of the call's list -- no compaction -- and counts its points with a layer;
 *   k_bev_score    the hot path.  A workgroup per (op, yaw), a thread per shift (sx fastest).  The op's grid is copied into the
 *                  middle of a (2 half + 2 sh)^2 byte LDS array whose border is zero, so that no lookup needs a bounds test.  The
 *                  query list goes by in chunks of 1024: every thread rotates and bins its share of the chunk and stages one u32
 *                  per point (the byte offset of the unshifted cell | layer << 24; a point that is not used gets layer 8, a bit
 *                  no byte has, at an offset every shift may read); then every thread walks the staged entries -- the entry is a
 *                  broadcast read, four entries per ds_read_b128 --, reads ONE byte at offset + sy * W + sx and adds the layer's
 *                  bit to a register.  The lanes of a read group touch 32 consecutive bytes (8 banks, 4 lanes per dword): no bank
 *                  conflict.  The walk is unrolled, so the reads of a group are in flight together behind counted waits;
 *   k_bev_peak     a workgroup per op: the maximum of (score << 32 | ~flat index), which is the tie rule, then the best score
 *                  outside the exclusion window.
 * Scores are integers counted in registers and stored once: an op's volume is the same bits alone, in any batch, on any repetition.
 * ll_bev_match enqueues one table upload, one fill (grids and query counts), the three launches and the copy of the peak records,
 * and synchronises ONCE.
 */
#include "ll_keyframes.h"
#include "ll_map_export.h"
#include "ll_map_search.h"
#include "ll_pose_math.h"
#include "ll_tiles.h"
#include <cmath>

#define BEV_TILE 1024
#define BEV_CHUNK 1024                                                /* staged entries: the first 4096 bytes of the dynamic LDS */
#define BEV_LDS_MAX (160 * 1024)

struct BevCfg { int half, sh; float inv, invz, zmin; };
/* off: the cloud's first point in the pool; pose, anchor: rows of the pose table; qbase: the cloud's first entry in the query list, -1: a target cloud */
struct BevSeg { long long off; int cnt; unsigned tile0; int pose, anchor, op, qbase; };
struct BevOpDev { int qbase, qcount, vbase, n_yaws; };               /* vbase: the op's first yaw row in the volume */
struct BevYaw { int op, j; float c, s; };

__global__ __launch_bounds__(256) void k_bev_prepare(const float4 *__restrict__ pool, const BevSeg *__restrict__ seg, int nseg, const double *__restrict__ poses,
                                                     BevCfg c, unsigned *grids, int *nq, float2 *__restrict__ qxy, signed char *__restrict__ qlay)
{
    const BevSeg s = seg[ll_tile_find(seg, nseg, blockIdx.x)];
    const int first = (int)(blockIdx.x - s.tile0) * BEV_TILE, n = min(BEV_TILE, s.cnt - first);
    const float4 *src = pool + s.off + first;
    const int kp = __builtin_amdgcn_readfirstlane(s.pose), ka = __builtin_amdgcn_readfirstlane(s.anchor);
    double PF[7], PA[7];
    for (int k = 0; k < 7; ++k) { PF[k] = poses[(size_t)kp * 7 + k]; PA[k] = poses[(size_t)ka * 7 + k]; }
    const int G = 2 * c.half;
    unsigned *grid = grids + (size_t)s.op * ((size_t)G * G / 4);
    const float lo = (float)-c.half, hi = (float)(c.half - 1);
    float4 po[BEV_TILE / 256];
#pragma unroll
    for (int k = 0; k < BEV_TILE / 256; ++k) po[k] = src[min(k * 256 + (int)threadIdx.x, n - 1)];
    int with_layer = 0;
#pragma unroll
    for (int k = 0; k < BEV_TILE / 256; ++k) {
        const int i = k * 256 + (int)threadIdx.x;
        float wx, wy, wz, lx, ly, lz;
        ll_map_to_world(PF, po[k], wx, wy, wz);
        vis_world_to_frame(PA, wx, wy, wz, lx, ly, lz);
        const bool finite = __builtin_isfinite(lx) && __builtin_isfinite(ly) && __builtin_isfinite(lz);
        const float fl = floorf((lz - c.zmin) * c.invz);
        const bool layer = i < n && finite && fl >= 0.0f && fl <= 7.0f;
        if (s.qbase < 0) {
            const float fx = floorf(lx * c.inv), fy = floorf(ly * c.inv);
            if (layer && fx >= lo && fx <= hi && fy >= lo && fy <= hi) {
                const int b = ((int)fy + c.half) * G + (int)fx + c.half;
                atomicOr(&grid[b >> 2], 1u << ((b & 3) * 8 + (int)fl));
            }
        } else if (i < n) {
            qxy[s.qbase + first + i] = make_float2(lx, ly);
            qlay[s.qbase + first + i] = (signed char)(layer ? (int)fl : -1);
            with_layer += layer ? 1 : 0;
        }
    }
    if (s.qbase >= 0) {                                               /* uniform per workgroup: whole waves come here */
        for (int d = 32; d > 0; d >>= 1) with_layer += __shfl_down(with_layer, d);
        if ((threadIdx.x & 63) == 0 && with_layer > 0) atomicAdd(&nq[s.op], with_layer);
    }
}

/* grid: one workgroup per row of the yaw table; (2 sh)^2 threads; dynamic LDS: BEV_CHUNK * 4 + (2 half + 2 sh)^2 bytes */
__global__ __launch_bounds__(1024) void k_bev_score(const unsigned char *__restrict__ grids, const float2 *__restrict__ qxy, const signed char *__restrict__ qlay,
                                                    const BevOpDev *__restrict__ optab, const BevYaw *__restrict__ yawtab, BevCfg c, int *__restrict__ volume)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bev_lds[];
    unsigned *stage = (unsigned *)bev_lds;
    unsigned char *cells = bev_lds + BEV_CHUNK * 4;
    const BevYaw y = yawtab[blockIdx.x];
    const BevOpDev o = optab[y.op];
    const int G = 2 * c.half, S = 2 * c.sh, W = G + S, nt = S * S, tid = (int)threadIdx.x;
    for (int i = tid; i < W * W / 4; i += nt) ((unsigned *)cells)[i] = 0u;           /* W is even: W * W is a multiple of 4 */
    __syncthreads();
    const unsigned *g = (const unsigned *)(grids + (size_t)y.op * ((size_t)G * G));
    for (int w = tid; w < G * G / 4; w += nt) {
        const unsigned v = g[w];
        if (v == 0u) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const unsigned byte = (v >> (8 * b)) & 255u;
            const int idx = 4 * w + b, row = idx / G, col = idx - row * G;
            if (byte) cells[(row + c.sh) * W + col + c.sh] = (unsigned char)byte;
        }
    }
    __syncthreads();
    const int sy = tid / S - c.sh, sx = tid - (tid / S) * S - c.sh;
    const int mine = sy * W + sx;                                    /* + an entry's offset: never negative (the border is sh wide) */
    const unsigned unused = (unsigned)(c.sh * W + c.sh) | (8u << 24);
    const float lo = (float)-c.half, hi = (float)(c.half - 1);
    int acc = 0;
    for (int base = 0; base < o.qcount; base += BEV_CHUNK) {
        for (int i = tid; i < BEV_CHUNK; i += nt) {
            unsigned e = unused;
            const int p = base + i;
            if (p < o.qcount) {
                const int layer = qlay[o.qbase + p];
                const float2 q = qxy[o.qbase + p];
                const float xr = y.c * q.x - y.s * q.y, yr = y.s * q.x + y.c * q.y;
                const float fx = floorf(xr * c.inv), fy = floorf(yr * c.inv);
                if (layer >= 0 && fx >= lo && fx <= hi && fy >= lo && fy <= hi)
                    e = (unsigned)(((int)fy + c.half + c.sh) * W + (int)fx + c.half + c.sh) | ((unsigned)layer << 24);
            }
            stage[i] = e;
        }
        __syncthreads();
        const int quads = (min(BEV_CHUNK, o.qcount - base) + 3) / 4;
        const uint4 *s4 = (const uint4 *)stage;
#pragma unroll 4
        for (int k = 0; k < quads; ++k) {
            const uint4 e = s4[k];
            acc += (int)((cells[mine + (int)(e.x & 0xffffffu)] >> (e.x >> 24)) & 1u);
            acc += (int)((cells[mine + (int)(e.y & 0xffffffu)] >> (e.y >> 24)) & 1u);
            acc += (int)((cells[mine + (int)(e.z & 0xffffffu)] >> (e.z >> 24)) & 1u);
            acc += (int)((cells[mine + (int)(e.w & 0xffffffu)] >> (e.w >> 24)) & 1u);
        }
        __syncthreads();
    }
    volume[(size_t)(o.vbase + y.j) * nt + tid] = acc;
}

/* grid: one workgroup per op.  rec[op] = (score, second, flat index of the best, n_query) */
__global__ __launch_bounds__(256) void k_bev_peak(const int *__restrict__ volume, const BevOpDev *__restrict__ optab, const int *__restrict__ nq, int S,
                                                  int excl_yaw, int excl_shift, int *__restrict__ rec)
{
    __shared__ unsigned long long best_of[256];
    __shared__ int second_of[256];
    const BevOpDev o = optab[blockIdx.x];
    const int per = S * S, n = o.n_yaws * per, tid = (int)threadIdx.x;
    const int *v = volume + (size_t)o.vbase * per;
    unsigned long long best = 0ull;                                  /* below every real key: a real key's low word is ~index > 0 */
    for (int i = tid; i < n; i += 256) best = max(best, ((unsigned long long)(unsigned)v[i] << 32) | (unsigned long long)(0xffffffffu - (unsigned)i));
    best_of[tid] = best;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) best_of[tid] = max(best_of[tid], best_of[tid + d]);
        __syncthreads();
    }
    best = best_of[0];
    const int at = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
    const int bj = at / per, by = (at - bj * per) / S, bx = at - bj * per - by * S;
    int second = -1;
    for (int i = tid; i < n; i += 256) {
        const int j = i / per, yy = (i - j * per) / S, xx = i - j * per - yy * S;
        if (abs(j - bj) > excl_yaw || abs(xx - bx) > excl_shift || abs(yy - by) > excl_shift) second = max(second, v[i]);
    }
    second_of[tid] = second;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) second_of[tid] = max(second_of[tid], second_of[tid + d]);
        __syncthreads();
    }
    if (tid == 0) {
        int *r = rec + (size_t)blockIdx.x * 4;
        r[0] = (int)(best >> 32); r[1] = second_of[0]; r[2] = at; r[3] = nq[blockIdx.x];
    }
}

/* ------------------------------------------------------------------ host side */
#define BEV_HIP(call) LL_HIP_CHECK(ll_fail, b, "bev: ", call, #call)

static size_t bev_lds_bytes(int half, int sh) { const size_t W = (size_t)(2 * half + 2 * sh); return W * W + BEV_CHUNK * 4; }

extern "C" void ll_bev_default_params(ll_bev_params *p)
{
    if (!p) return;
    p->cell = 0.5f; p->half = 128; p->shift_half = 16; p->z_min = -1.0f; p->z_layer = 1.0f; p->excl_yaw = 1; p->excl_shift = 2;
    p->max_ops = 64; p->max_yaws = 16; p->max_points = 1ll << 21;
}

extern "C" int ll_bev_create(ll_keyframes *kf, const ll_bev_params *p, ll_bev **out)
{
    if (!kf || !p || !out) return LL_ERR_ARG;
    *out = nullptr;
    if (!std::isfinite(p->cell) || !(p->cell > 0.0f) || !std::isfinite(p->z_layer) || !(p->z_layer > 0.0f) || !std::isfinite(p->z_min) || p->half < 1 || p->half > 512 ||
        p->shift_half < 1 || p->shift_half > 16 || p->excl_yaw < 0 || p->excl_shift < 0 || p->max_ops < 1 || p->max_ops > 4096 || p->max_yaws < 1 || p->max_yaws > 64 ||
        p->max_points < 1 || p->max_points > (1ll << 30))
        return llkf_create_err(kf, LL_ERR_ARG, "bev: bad parameters (cell, z_layer finite and > 0, z_min finite, half in 1 .. 512, shift_half in 1 .. 16, excl_yaw, excl_shift >= 0, "
                                          "max_ops in 1 .. 4096, max_yaws in 1 .. 64, max_points in 1 .. 2^30)");
    if (bev_lds_bytes(p->half, p->shift_half) > (size_t)BEV_LDS_MAX)
        return llkf_create_err(kf, LL_ERR_ARG, "bev: (2 half + 2 shift_half)^2 + 4096 = " + std::to_string(bev_lds_bytes(p->half, p->shift_half)) + " bytes do not fit the 160 KiB of LDS");
    ll_ctx *ctx = kf->ctx;
    if (hipSetDevice(ctx->device) != hipSuccess) return llkf_create_err(kf, LL_ERR_HIP, "bev: hipSetDevice failed");
    ll_bev *b = new ll_bev();
    b->follow(kf); b->p = *p;
    bool ok = true;
    for (int k = 0; ok && k < 4; ++k) ok = hipEventCreate(&b->ev[k]) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ll_bev_destroy(b);
        return llkf_create_err(kf, LL_ERR_HIP, "bev: hipEventCreate failed");
    }
    *out = b;
    return LL_OK;
}

extern "C" void ll_bev_destroy(ll_bev *b)
{
    if (!b) return;
    b->release();
    if (b->d_mem) (void)hipFree(b->d_mem);
    for (int k = 0; k < 4; ++k) if (b->ev[k]) (void)hipEventDestroy(b->ev[k]);
    delete b;
}

extern "C" const char *ll_bev_last_error(const ll_bev *b) { return b ? b->err.c_str() : "null bev"; }

static int bev_stale(ll_bev *b) { return b->stale("bev: the store was reset since the object was made: call ll_bev_reset"); }

/* the two lists of an op: target, query */
static LLKfList bev_side(const ll_bev_op &o, int side)
{
    if (side) return {o.n_query, o.query, o.query_poses_w7, "query"};
    return {o.n_target, o.target, o.target_poses_w7, "target"};
}

extern "C" int ll_bev_reset(ll_bev *b)
{
    if (!b) return LL_ERR_ARG;
    b->epoch = b->kf->n_reset; b->last_vbase.clear(); b->last_nyaws.clear();
    for (int k = 0; k < 3; ++k) { b->ms[k] = 0.0; b->counts[k] = 0; }
    return LL_OK;
}

extern "C" int ll_bev_match(ll_bev *b, const ll_bev_op *ops, int n_ops, ll_bev_result *out)
{
    if (!b) return LL_ERR_ARG;
    if (!ops || !out) return b->fail(LL_ERR_ARG, "bev: ops or out is NULL");
    if (n_ops < 1 || n_ops > b->p.max_ops) return b->fail(LL_ERR_ARG, "bev: n_ops = " + std::to_string(n_ops) + " is outside 1 .. max_ops = " + std::to_string(b->p.max_ops));
    const ll_keyframes *kf = b->kf;
    const ll_keyframe_info *tab = kf->tab.data();
    const int size = (int)kf->tab.size();
    /* ---- every refusal before anything is enqueued */
    long long n_points = 0, n_rows = 0;
    for (int i = 0; i < n_ops; ++i) {
        const ll_bev_op &o = ops[i];
        const std::string who = "bev: op " + std::to_string(i) + ": ";
        if (o.n_yaws < 1 || o.n_yaws > b->p.max_yaws) return b->fail(LL_ERR_ARG, who + "n_yaws = " + std::to_string(o.n_yaws) + " is outside 1 .. max_yaws = " + std::to_string(b->p.max_yaws));
        if (!std::isfinite(o.yaw0) || !std::isfinite(o.yaw_step) || !std::isfinite(o.yaw0 + (double)(o.n_yaws - 1) * o.yaw_step)) return b->fail(LL_ERR_ARG, who + "a yaw is not finite");
        for (int side = 0; side < 2; ++side) {
            const LLKfList list = bev_side(o, side);
            long long pts;
            if (list.n < 1 || !list.ids) return b->fail(LL_ERR_ARG, who + "the " + list.side + " side has no frame or its list is NULL");
            if (llkf_check(tab, size, list, LLKF_DUP_ALLOWED, nullptr, i, who, &b->err, &pts)) return LL_ERR_ARG;
            n_points += pts;
        }
        n_rows += o.n_yaws;
    }
    if (n_points > b->p.max_points) return b->fail(LL_ERR_CAPACITY, "bev: " + std::to_string(n_points) + " listed points, max_points is " + std::to_string(b->p.max_points));
    int rc = bev_stale(b); if (rc) return rc;
    /* ---- the tables: clouds (query clouds of an op back to back in the list), poses, ops, yaws */
    const int S = 2 * b->p.shift_half, G = 2 * b->p.half;
    std::vector<BevSeg> segs;
    std::vector<double> poses;
    std::vector<BevOpDev> optab((size_t)n_ops);
    std::vector<BevYaw> yawtab; yawtab.reserve((size_t)n_rows);
    std::vector<int> vbase((size_t)n_ops), nyaws((size_t)n_ops);
    LLTiler tiles{BEV_TILE};
    long long n_query_points = 0;
    for (int i = 0; i < n_ops; ++i) {
        const ll_bev_op &o = ops[i];
        optab[i].qbase = (int)n_query_points; optab[i].vbase = (int)yawtab.size(); optab[i].n_yaws = o.n_yaws;
        for (int side = 0; side < 2; ++side) {
            const LLKfList list = bev_side(o, side);
            const int anchor = (int)(poses.size() / 7);
            for (int f = 0; f < list.n; ++f) {
                const double *P = llkf_pose(tab, list, f);
                poses.insert(poses.end(), P, P + 7);
                for (int w = 0; w < 2; ++w) {
                    const LLKfCloud cl = llkf_cloud(tab, kf->cap[0], list.ids[f], w);
                    if (cl.cnt <= 0) continue;
                    segs.push_back({cl.off, cl.cnt, tiles.take(cl.cnt), anchor + f, anchor, i, side ? (int)n_query_points : -1});
                    if (side) n_query_points += cl.cnt;
                }
            }
        }
        optab[i].qcount = (int)n_query_points - optab[i].qbase;
        vbase[i] = optab[i].vbase; nyaws[i] = o.n_yaws;
        for (int j = 0; j < o.n_yaws; ++j) {
            const double yaw = o.yaw0 + (double)j * o.yaw_step;
            yawtab.push_back({i, j, (float)std::cos(yaw), (float)std::sin(yaw)});
        }
    }
    if (!tiles.fits()) return b->fail(LL_ERR_CAPACITY, "bev: too many tiles for one call");
    /* ---- the buffer: grids | query counts | peak records | volume | query (x, y) | query layers */
    const size_t grid_bytes = (size_t)G * G, fill_bytes = (size_t)n_ops * grid_bytes + (size_t)n_ops * 4;
    const size_t at_nq = (size_t)n_ops * grid_bytes, at_rec = ll_up256(fill_bytes), at_vol = ll_up256(at_rec + (size_t)n_ops * 16);
    const size_t at_qxy = ll_up256(at_vol + (size_t)n_rows * S * S * 4), at_qlay = ll_up256(at_qxy + (size_t)n_query_points * 8);
    const size_t need = at_qlay + (size_t)n_query_points + 16;
    hipStream_t st = b->ctx->stream;
    BEV_HIP(hipSetDevice(b->ctx->device));
    if (need > b->cap_mem) {
        b->last_vbase.clear(); b->last_nyaws.clear();                 /* the last call's volume goes with the old buffer */
        BEV_HIP(hipStreamSynchronize(st));
        if (b->d_mem) (void)hipFree(b->d_mem);
        b->d_mem = nullptr; b->cap_mem = 0;
        const size_t cap = std::max(need, (size_t)1 << 20);
        void *mem = nullptr;
        if (hipMalloc(&mem, cap) != hipSuccess) { (void)hipGetLastError(); return b->fail(LL_ERR_HIP, "bev: no device memory for " + std::to_string(cap) + " bytes"); }
        b->d_mem = (unsigned char *)mem; b->cap_mem = cap;
    }
    std::vector<unsigned char> blob;
    const size_t at_seg = ll_blob_put(blob, segs), at_pose = ll_blob_put(blob, poses), at_op = ll_blob_put(blob, optab), at_yaw = ll_blob_put(blob, yawtab);
    const unsigned char *d_blob = (const unsigned char *)llx_stage_bytes(b->X, blob.data(), blob.size(), st, b->err);
    if (!d_blob) return LL_ERR_HIP;
    int *pin = (int *)ll_pinned_scratch((size_t)n_ops * 16);
    if (!pin) return b->fail(LL_ERR_HIP, "bev: no page-locked scratch");
    b->last_vbase.clear(); b->last_nyaws.clear();                     /* the volume is being overwritten from here on */
    BevCfg c;
    c.half = b->p.half; c.sh = b->p.shift_half; c.zmin = b->p.z_min;
    c.inv = (float)(1.0 / (double)b->p.cell); c.invz = (float)(1.0 / (double)b->p.z_layer);
    unsigned char *m = b->d_mem;
    const BevOpDev *d_op = (const BevOpDev *)(d_blob + at_op);
    const size_t lds = bev_lds_bytes(c.half, c.sh);
    static size_t lds_set[LL_MAX_DEVICES] = {};
    ll_ensure_dynamic_lds(k_bev_score, lds, lds_set);
    BEV_HIP(hipMemsetAsync(m, 0, fill_bytes, st));
    BEV_HIP(hipEventRecord(b->ev[0], st));
    if (tiles.next > 0)
        hipLaunchKernelGGL(k_bev_prepare, dim3((unsigned)tiles.next), dim3(256), 0, st, (const float4 *)kf->pool, (const BevSeg *)(d_blob + at_seg), (int)segs.size(),
                           (const double *)(d_blob + at_pose), c, (unsigned *)m, (int *)(m + at_nq), (float2 *)(m + at_qxy), (signed char *)(m + at_qlay));
    BEV_HIP(hipEventRecord(b->ev[1], st));
    hipLaunchKernelGGL(k_bev_score, dim3((unsigned)n_rows), dim3((unsigned)(S * S)), lds, st, (const unsigned char *)m, (const float2 *)(m + at_qxy),
                       (const signed char *)(m + at_qlay), d_op, (const BevYaw *)(d_blob + at_yaw), c, (int *)(m + at_vol));
    BEV_HIP(hipEventRecord(b->ev[2], st));
    hipLaunchKernelGGL(k_bev_peak, dim3((unsigned)n_ops), dim3(256), 0, st, (const int *)(m + at_vol), d_op, (const int *)(m + at_nq), S, b->p.excl_yaw,
                       b->p.excl_shift, (int *)(m + at_rec));
    BEV_HIP(hipEventRecord(b->ev[3], st));
    BEV_HIP(hipGetLastError());
    BEV_HIP(hipMemcpyAsync(pin, m + at_rec, (size_t)n_ops * 16, hipMemcpyDeviceToHost, st));
    BEV_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 3; ++k) b->ms[k] = ll_event_ms(b->ev[k], b->ev[k + 1], 0.0);
    b->counts[0] = n_ops; b->counts[1] = n_points; b->counts[2] = n_rows * S * S;
    b->at_volume = at_vol; b->last_vbase = vbase; b->last_nyaws = nyaws;
    for (int i = 0; i < n_ops; ++i) {
        const int *r = pin + (size_t)i * 4;
        ll_bev_result &o = out[i];
        const int per = S * S, j = r[2] / per, ry = (r[2] - j * per) / S, rx = r[2] - j * per - ry * S;
        o.score = r[0]; o.second = r[1]; o.iyaw = j; o.sx = rx - b->p.shift_half; o.sy = ry - b->p.shift_half; o.n_query = r[3];
        o.yaw = ops[i].yaw0 + (double)j * ops[i].yaw_step;
        o.D_w7[0] = 0.0; o.D_w7[1] = 0.0; o.D_w7[2] = std::sin(o.yaw / 2.0); o.D_w7[3] = std::cos(o.yaw / 2.0);
        o.D_w7[4] = (double)o.sx * (double)b->p.cell; o.D_w7[5] = (double)o.sy * (double)b->p.cell; o.D_w7[6] = 0.0;
    }
    return LL_OK;
}

/* bytes at `at` of the buffer to the host; one synchronisation */
static int bev_read(ll_bev *b, size_t at, size_t bytes, void *dst)
{
    const LLKfRange range = {b->d_mem + at, bytes, dst};
    return b->read("bev: ", &range, 1);
}

static int bev_last_op(ll_bev *b, int op, const void *dst)
{
    if (!dst) return b->fail(LL_ERR_ARG, "bev: the output pointer is NULL");
    const int rc = bev_stale(b); if (rc) return rc;
    if (op < 0 || op >= (int)b->last_nyaws.size()) return b->fail(LL_ERR_ARG, "bev: the last call had " + std::to_string(b->last_nyaws.size()) + " ops, there is no op " + std::to_string(op));
    return LL_OK;
}

extern "C" int ll_bev_volume(ll_bev *b, int op, int *scores)
{
    if (!b) return LL_ERR_ARG;
    const int rc = bev_last_op(b, op, scores); if (rc) return rc;
    const size_t per = (size_t)4 * b->p.shift_half * b->p.shift_half * sizeof(int);
    return bev_read(b, b->at_volume + (size_t)b->last_vbase[op] * per, (size_t)b->last_nyaws[op] * per, scores);
}

extern "C" int ll_bev_grid(ll_bev *b, int op, unsigned char *cells)
{
    if (!b) return LL_ERR_ARG;
    const int rc = bev_last_op(b, op, cells); if (rc) return rc;
    const size_t bytes = (size_t)4 * b->p.half * b->p.half;
    return bev_read(b, (size_t)op * bytes, bytes, cells);
}

extern "C" int ll_bev_timing(const ll_bev *b, double *ms, long long *counts)
{
    return b ? llkf_timing(b->ms, b->counts, 3, ms, counts) : LL_ERR_ARG;
}

/* ---- T0 = P_c o D o P_q^-1, plain host f64 in the Eigen form (the header spells the operations; ll_pose_math.h is their text) */
extern "C" int ll_bev_guess(const double *Pc_w7, const double *D_w7, const double *Pq_w7, double *T0_w7)
{
    if (!Pc_w7 || !D_w7 || !Pq_w7 || !T0_w7) return LL_ERR_ARG;
    double T[7];
    ll_pose_inverse(Pq_w7, T);
    ll_pose_compose(D_w7, T, T);
    ll_pose_compose(Pc_w7, T, T0_w7);
    return LL_OK;
}
