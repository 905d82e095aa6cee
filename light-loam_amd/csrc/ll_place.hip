/*
 * ll_place.hip -- ll_places: Scan Context place descriptors (Kim & Kim, IROS 2018) of resident scans and the exhaustive, exact
 * search of every query against every stored place.  Not in the reference; the contract is in include/lightloam_hip.h.
 *
 * Per place the database holds, in HBM,
 *   desc   [20][60]  the descriptor, desc[ring][sector] = max (z + z_offset) of the bin's points, 0 for a bin without points;
 *   unit   [20][64]  the match-ready form: every column (sector) scaled to unit length, ring-major with the 60 columns padded
 *                    to 64 by zeros -- a row of it is what one f32-input MFMA operand register of a wave reads;
 *   mask             bit j: column j is not empty (its norm is not 0).
 *   k_pl_describe  one workgroup per place of the call: the points of the slot's laserCloud (ring rows at stride ring_cap, as mode
 *                  2 of k_deskew walks them) or of an uploaded cloud go into 1200 LDS cells with an integer max over an
 *                  order-preserving key of the float.  A maximum does not depend on the order, so the descriptor is bit-determined;
 *   k_pl_prepare   64 lanes per place, one column each: the norm summed over rings 0 .. 19 in that order, the scaled column, the mask.
 *                  add_slots, add_points and upload all go through it.
 *   k_pl_gram      a wave takes one (query, candidate) pair at a time: G = Uq^T Uc, 64 x 64 with K = 20, as 2 x 2 tiles of 32 x 32 on
 *                  v_mfma_f32_32x32x2_f32 (40 instructions; exact f32, a k-ordered fmaf chain); the next candidate's operands are
 *                  loaded as soon as the 40 are issued, so they travel while this tile is summed.  The tile is staged through LDS
 *                  at a row stride of 61 floats (odd: the 60 lanes of a wrapped-diagonal read fall on 60 banks) and lane s sums
 *                  G[(j + s) mod 60][j] over j = 0 .. 59 in that order.  An empty column's unit form is all zero, so its terms are
 *                  exact zeros and only `count` needs the masks.  The argmin over the 60 shifts is a butterfly on (d, s), a total
 *                  order.  No step depends on which wave, workgroup or launch a pair falls in: its (distance, shift) has the
 *                  same bits alone or inside any batch.
 *   k_pl_select    one workgroup per query: every thread keeps the 8 best of its share of the row by (distance, id), then K
 *                  rounds of a workgroup argmin over the lists' heads.
 * ll_places_distances and ll_places_match synchronise with the host ONCE, for their results.
 */
#include "ll_internal.h"
#include <climits>
#include <cmath>

#define PL_RINGS 20
#define PL_SECT 60
#define PL_DESC (PL_RINGS * PL_SECT)
#define PL_UW 64                              /* columns of a ring row of the unit form */
#define PL_UNIT (PL_RINGS * PL_UW)
#define PL_LS 61                              /* LDS row stride of the staged Gram matrix */
#define PL_WAVES 4
#define PL_CPW 16                             /* candidates per wave of a k_pl_gram workgroup */
#define PL_CHUNK (PL_WAVES * PL_CPW)
#define PL_KMAX 8
#define PL_MAX_PAIRS (1ll << 26)
#define PL_TWO_PI 6.2831855f
#define PL_SECT_PER_RAD 9.549296585513721f    /* rounds to the float nearest to 60 / (2 pi) */

typedef float pl_f32x16 __attribute__((ext_vector_type(16)));

struct ll_places {
    ll_ctx *ctx = nullptr;
    ll_places_params p;
    int size = 0;
    float *d_desc = nullptr, *d_unit = nullptr;
    unsigned long long *d_mask = nullptr;
    /* grown to the need of a call, kept */
    void *d_in = nullptr; size_t cap_in = 0;          /* an add's slot list or cloud, a match's c_end */
    float *d_dist = nullptr; size_t cap_dist = 0;     /* [nq][nc] */
    unsigned char *d_shift = nullptr; size_t cap_shift = 0;
    unsigned char *d_sel = nullptr; size_t cap_sel = 0;   /* [nq][K] ids, distances, shifts */
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   /* add: 0, 1; match: 2, 3, 4 */
    bool add_pending = false;
    double ms[3] = {0.0, 0.0, 0.0};
    long long counts[2] = {0, 0};
    std::string err;
};

/* an int whose order is the float's (-inf .. +inf) */
__device__ __forceinline__ int pl_key(float v) { const int i = __float_as_int(v); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float pl_unkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__device__ __forceinline__ void pl_bin(const float4 p, float max_radius, float w, float z_offset, int *key)
{
    const float r = sqrtf(p.x * p.x + p.y * p.y);
    if (!(r < max_radius)) return;                                 /* also a NaN */
    const int i = min(PL_RINGS - 1, (int)(r / w));
    float a = ll_atan2f(p.y, p.x);
    if (a < 0.0f) a += PL_TWO_PI;
    const int j = min(PL_SECT - 1, (int)(a * PL_SECT_PER_RAD));
    atomicMax(&key[i * PL_SECT + j], pl_key(p.z + z_offset));
}

/* place blockIdx.x of the call: slot slots[blockIdx.x]'s laserCloud, or (pts != NULL, one place) the n_pts points at pts */
__global__ __launch_bounds__(256) void k_pl_describe(LLView V, const int *slots, const float4 *pts, int n_pts, float *desc,
                                                     float max_radius, float w, float z_offset)
{
    __shared__ int key[PL_DESC];
    const int tid = threadIdx.x;
    for (int i = tid; i < PL_DESC; i += 256) key[i] = INT_MIN;
    __syncthreads();
    if (pts) {
        for (int i = tid; i < n_pts; i += 256) pl_bin(pts[i], max_radius, w, z_offset, key);
    } else {
        const int s = slots[blockIdx.x];
        const ScanHdr h = V.hdr[s];
        if (h.status == 0 && h.n > 0) {                            /* a refused or empty slot: the all-zero descriptor */
            const int *ro = V.ring_off + (size_t)s * (V.R + 1);
            for (int r = 0; r < V.R; ++r) {
                const int off = ro[r];
                const int n = off >= 0 ? min(ro[r + 1] - off, V.ring_cap) : 0;
                const float4 *base = V.cloud + (size_t)s * V.CS + (size_t)r * V.ring_cap;
                for (int i = tid; i < n; i += 256) pl_bin(base[i], max_radius, w, z_offset, key);
            }
        }
    }
    __syncthreads();
    float *d = desc + (size_t)blockIdx.x * PL_DESC;
    for (int i = tid; i < PL_DESC; i += 256) d[i] = key[i] == INT_MIN ? 0.0f : pl_unkey(key[i]);
}

/* the match-ready form of place first + blockIdx.x: lane j takes column j */
__global__ __launch_bounds__(64) void k_pl_prepare(const float *desc, float *unit, unsigned long long *mask, int first)
{
    const size_t p = (size_t)first + blockIdx.x;
    const int j = threadIdx.x;
    const float *d = desc + p * PL_DESC;
    float col[PL_RINGS], n2 = 0.0f;
#pragma unroll
    for (int k = 0; k < PL_RINGS; ++k) { col[k] = j < PL_SECT ? d[k * PL_SECT + j] : 0.0f; n2 += col[k] * col[k]; }
    const float nrm = sqrtf(n2);
    const bool full = j < PL_SECT && nrm != 0.0f;
#pragma unroll
    for (int k = 0; k < PL_RINGS; ++k) unit[p * PL_UNIT + k * PL_UW + j] = full ? col[k] / nrm : 0.0f;
    const unsigned long long m = __ballot(full);
    if (j == 0) mask[p] = m;
}

/* workgroup b: query q0 + b / nchunk against candidates c0 + (b % nchunk) * PL_CHUNK + 4 it + wave, it = 0 .. PL_CPW - 1.
 * MFMA lane maps (32x32x2 f32): lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; register g of the
 * accumulator is D[(g & 3) + 8 (g >> 2) + 4 (l >> 5)][l & 31].  A = Uq^T (row i = the query's column), B = Uc. */
__global__ __launch_bounds__(64 * PL_WAVES) void k_pl_gram(const float *unit, const unsigned long long *mask, int q0, int c0, int nc,
                                                           int nchunk, float *dist, unsigned char *shift)
{
    __shared__ float G[PL_WAVES][PL_SECT * PL_LS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x / nchunk, cbase = (blockIdx.x % nchunk) * PL_CHUNK;
    const int l31 = lane & 31, lh = lane >> 5;
    const float *uq = unit + (size_t)(q0 + q) * PL_UNIT;
    float a[2][PL_RINGS / 2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int kk = 0; kk < PL_RINGS / 2; ++kk) a[h][kk] = uq[(2 * kk + lh) * PL_UW + 32 * h + l31];
    const unsigned long long mq = mask[q0 + q];
    float *g = G[wave];
    /* the candidate of round `it` (an index past the last one reads the last one again; its result is not written) */
    auto place = [&](int it) { return (size_t)c0 + min(cbase + it * PL_WAVES + wave, nc - 1); };
    float b[2][PL_RINGS / 2];
    auto load_b = [&](size_t pc) {
        const float *uc = unit + pc * PL_UNIT;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int kk = 0; kk < PL_RINGS / 2; ++kk) b[h][kk] = uc[(2 * kk + lh) * PL_UW + 32 * h + l31];
    };
    load_b(place(0));
    unsigned long long mc_next = mask[place(0)];
    for (int it = 0; it < PL_CPW; ++it) {
        if (cbase + it * PL_WAVES >= nc) break;                    /* the same for the whole workgroup */
        const int c = cbase + it * PL_WAVES + wave;
        const bool live = c < nc;
        const unsigned long long mc = mc_next;
        pl_f32x16 acc[2][2];
#pragma unroll
        for (int hi = 0; hi < 2; ++hi)
#pragma unroll
            for (int hj = 0; hj < 2; ++hj)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[hi][hj][r] = 0.0f;
#pragma unroll
        for (int kk = 0; kk < PL_RINGS / 2; ++kk)
#pragma unroll
            for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                for (int hj = 0; hj < 2; ++hj) acc[hi][hj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[hi][kk], b[hj][kk], acc[hi][hj], 0, 0, 0);
        if (it + 1 < PL_CPW) {                                     /* the next candidate's operands travel while this tile is summed */
            load_b(place(it + 1));
            mc_next = mask[place(it + 1)];
        }
#pragma unroll
        for (int hi = 0; hi < 2; ++hi)
#pragma unroll
            for (int hj = 0; hj < 2; ++hj)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = 32 * hi + (r & 3) + 8 * (r >> 2) + 4 * lh, col = 32 * hj + l31;
                    if (row < PL_SECT && col < PL_SECT) g[row * PL_LS + col] = acc[hi][hj][r];
                }
        __syncthreads();
        /* lane s: d(s) from the wrapped diagonal G[(j + s) mod 60][j], j ascending */
        float d = INFINITY;
        int s = 64;
        if (lane < PL_SECT) {
            float sim = 0.0f;
            int row = lane;
            for (int j = 0; j < PL_SECT; ++j) {
                sim += g[row * PL_LS + j];
                row = row + 1 == PL_SECT ? 0 : row + 1;
            }
            const unsigned long long all = (1ull << PL_SECT) - 1ull;
            const unsigned long long rot = lane == 0 ? mq : (((mq >> lane) | (mq << (PL_SECT - lane))) & all);   /* bit j: the query's column (j + s) mod 60 */
            const int count = __popcll(rot & mc);
            d = count > 0 ? 1.0f - sim / (float)count : 1.0f;
            s = lane;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float d2 = __shfl_xor(d, o);
            const int s2 = __shfl_xor(s, o);
            if (d2 < d || (d2 == d && s2 < s)) { d = d2; s = s2; }
        }
        if (lane == 0 && live) {
            dist[(size_t)q * nc + c] = d;
            shift[(size_t)q * nc + c] = (unsigned char)(s < PL_SECT ? s : 0);
        }
        __syncthreads();                                           /* the tile is free again */
    }
}

__device__ __forceinline__ bool pl_less(float d2, int i2, float d, int i) { return d2 < d || (d2 == d && i2 < i); }

/* query blockIdx.x: the K best of its row of dist by (distance, candidate), of the candidates with id < c_end[q] */
__global__ __launch_bounds__(256) void k_pl_select(const float *dist, const unsigned char *shift, int nc, int c0, const int *c_end, int K,
                                                   int *oid, float *odist, unsigned char *oshift)
{
    __shared__ float ld[PL_KMAX * 256];
    __shared__ int li[PL_KMAX * 256];
    __shared__ float wd[4];
    __shared__ int wi[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    int vis = nc;
    if (c_end) { const long long v = (long long)c_end[q] - c0; vis = v < 0 ? 0 : (v < nc ? (int)v : nc); }
    const float *row = dist + (size_t)q * nc;
    float bd[PL_KMAX]; int bi[PL_KMAX];
#pragma unroll
    for (int k = 0; k < PL_KMAX; ++k) { bd[k] = INFINITY; bi[k] = INT_MAX; }
    for (int c = tid; c < vis; c += 256) {
        const float d = row[c];
        if (!(d < bd[PL_KMAX - 1])) continue;                      /* a thread's candidates ascend: a tie stays behind the earlier one */
        bd[PL_KMAX - 1] = d; bi[PL_KMAX - 1] = c;
#pragma unroll
        for (int k = PL_KMAX - 1; k > 0; --k)
            if (bd[k] < bd[k - 1]) { const float td = bd[k]; bd[k] = bd[k - 1]; bd[k - 1] = td; const int ti = bi[k]; bi[k] = bi[k - 1]; bi[k - 1] = ti; }
    }
#pragma unroll
    for (int k = 0; k < PL_KMAX; ++k) { ld[k * 256 + tid] = bd[k]; li[k * 256 + tid] = bi[k]; }
    int head = 0;
    for (int r = 0; r < K; ++r) {
        const float hd = head < PL_KMAX ? ld[head * 256 + tid] : INFINITY;
        const int hi = head < PL_KMAX ? li[head * 256 + tid] : INT_MAX;
        float d = hd; int i = hi;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float d2 = __shfl_xor(d, o);
            const int i2 = __shfl_xor(i, o);
            if (pl_less(d2, i2, d, i)) { d = d2; i = i2; }
        }
        if ((tid & 63) == 0) { wd[tid >> 6] = d; wi[tid >> 6] = i; }
        __syncthreads();
        d = wd[0]; i = wi[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) if (pl_less(wd[w], wi[w], d, i)) { d = wd[w]; i = wi[w]; }
        if (i != INT_MAX && hi == i) ++head;
        if (tid == 0) {
            const size_t o = (size_t)q * K + r;
            if (i != INT_MAX) { oid[o] = c0 + i; odist[o] = d; oshift[o] = shift[(size_t)q * nc + i]; }
            else { oid[o] = -1; odist[o] = INFINITY; oshift[o] = 0; }
        }
        __syncthreads();
    }
}

/* ------------------------------------------------------------------ host side */
static int pl_fail(ll_places *db, int code, const std::string &what) { db->err = what; return code; }

#define PL_HIP(call) LL_HIP_CHECK(pl_fail, db, "places: ", call, #call)

template <typename T>
static bool pl_grow(T *&ptr, size_t &cap, size_t bytes)
{
    if (bytes <= cap) return true;
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (ptr) (void)hipFree(ptr);                                   /* hipFree waits for the work that may still read it */
    ptr = (T *)p; cap = bytes;
    return true;
}

extern "C" void ll_places_default_params(ll_places_params *p, int capacity)
{
    if (!p) return;
    p->capacity = capacity; p->max_radius = 80.0f; p->z_offset = 2.0f;
}

extern "C" void ll_places_destroy(ll_places *db)
{
    if (!db) return;
    (void)hipSetDevice(db->ctx->device);
    for (void *p : {(void *)db->d_desc, (void *)db->d_unit, (void *)db->d_mask, db->d_in, (void *)db->d_dist, (void *)db->d_shift, (void *)db->d_sel})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : db->ev) if (e) (void)hipEventDestroy(e);
    delete db;
}

extern "C" int ll_places_create(ll_ctx *ctx, const ll_places_params *p, ll_places **out)
{
    if (!ctx || !out) return LL_ERR_ARG;
    *out = nullptr;
    if (!p || p->capacity < 1 || p->capacity > (1 << 24) || !(p->max_radius > 0.0f) || !std::isfinite(p->max_radius) || !std::isfinite(p->z_offset)) {
        ctx->err = "places: capacity outside 1 .. 2^24, or max_radius / z_offset not finite and positive";
        return LL_ERR_ARG;
    }
    LL_HIP(hipSetDevice(ctx->device));
    ll_places *db = new ll_places();
    db->ctx = ctx; db->p = *p;
    const size_t cap = (size_t)p->capacity;
    bool ok = hipMalloc((void **)&db->d_desc, cap * PL_DESC * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&db->d_unit, cap * PL_UNIT * sizeof(float)) == hipSuccess &&
              hipMalloc((void **)&db->d_mask, cap * sizeof(unsigned long long)) == hipSuccess;
    for (hipEvent_t &e : db->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ll_places_destroy(db);
        ctx->err = "places: allocation failed (" + std::to_string(cap * (PL_DESC + PL_UNIT) * sizeof(float)) + " bytes)";
        return LL_ERR_HIP;
    }
    *out = db;
    return LL_OK;
}

extern "C" const char *ll_places_last_error(const ll_places *db) { return db ? db->err.c_str() : "places: NULL handle"; }

extern "C" int ll_places_size(const ll_places *db) { return db ? db->size : LL_ERR_ARG; }

extern "C" int ll_places_reset(ll_places *db)
{
    if (!db) return LL_ERR_ARG;
    db->size = 0;
    return LL_OK;
}

/* describe (slots or cloud already in d_in) `count` places from `first`, then their match-ready form */
static int pl_describe(ll_places *db, int first, int count, const float4 *pts, int n_pts)
{
    hipStream_t st = db->ctx->stream;
    const float w = db->p.max_radius / 20.0f;
    PL_HIP(hipEventRecord(db->ev[0], st));
    hipLaunchKernelGGL(k_pl_describe, dim3((unsigned)count), dim3(256), 0, st, db->ctx->V, pts ? nullptr : (const int *)db->d_in, pts, n_pts,
                       db->d_desc + (size_t)first * PL_DESC, db->p.max_radius, w, db->p.z_offset);
    hipLaunchKernelGGL(k_pl_prepare, dim3((unsigned)count), dim3(64), 0, st, (const float *)db->d_desc, db->d_unit, db->d_mask, first);
    PL_HIP(hipEventRecord(db->ev[1], st));
    PL_HIP(hipGetLastError());
    db->add_pending = true; db->counts[0] = count;
    return LL_OK;
}

extern "C" int ll_places_add_slots(ll_places *db, const int *slots, int count, int *first_id)
{
    if (!db) return LL_ERR_ARG;
    if (count < 0 || (count > 0 && !slots)) return pl_fail(db, LL_ERR_ARG, "places: add_slots: count < 0 or slots is NULL");
    for (int i = 0; i < count; ++i)
        if (slots[i] < 0 || slots[i] >= db->ctx->p.batch) return pl_fail(db, LL_ERR_ARG, "places: add_slots: entry " + std::to_string(i) + " is no slot of the context");
    if ((long long)db->size + count > db->p.capacity) return pl_fail(db, LL_ERR_CAPACITY, "places: add_slots: " + std::to_string(db->size) + " + " + std::to_string(count) + " places exceed the capacity " + std::to_string(db->p.capacity));
    if (first_id) *first_id = db->size;
    if (count == 0) return LL_OK;
    PL_HIP(hipSetDevice(db->ctx->device));
    if (!pl_grow(db->d_in, db->cap_in, (size_t)count * sizeof(int))) return pl_fail(db, LL_ERR_HIP, "places: hipMalloc failed for the slot list");
    PL_HIP(hipMemcpyAsync(db->d_in, slots, (size_t)count * sizeof(int), hipMemcpyHostToDevice, db->ctx->stream));
    const int rc = pl_describe(db, db->size, count, nullptr, 0); if (rc) return rc;
    db->size += count;
    return LL_OK;
}

extern "C" int ll_places_add_points(ll_places *db, const ll_point *host, int n, int *id)
{
    if (!db) return LL_ERR_ARG;
    if (n < 0 || (n > 0 && !host)) return pl_fail(db, LL_ERR_ARG, "places: add_points: n < 0 or the cloud is NULL");
    if (db->size + 1 > db->p.capacity) return pl_fail(db, LL_ERR_CAPACITY, "places: add_points: the database is full (" + std::to_string(db->p.capacity) + " places)");
    if (id) *id = db->size;
    PL_HIP(hipSetDevice(db->ctx->device));
    if (!pl_grow(db->d_in, db->cap_in, (size_t)(n > 0 ? n : 1) * sizeof(float4))) return pl_fail(db, LL_ERR_HIP, "places: hipMalloc failed for the cloud");
    if (n > 0) PL_HIP(hipMemcpyAsync(db->d_in, host, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, db->ctx->stream));
    const int rc = pl_describe(db, db->size, 1, (const float4 *)db->d_in, n); if (rc) return rc;
    db->size += 1;
    return LL_OK;
}

extern "C" int ll_places_upload(ll_places *db, int first, int count, const float *desc1200)
{
    if (!db) return LL_ERR_ARG;
    if (first < 0 || count < 0 || first > db->size || (count > 0 && !desc1200)) return pl_fail(db, LL_ERR_ARG, "places: upload: first outside 0 .. size, count < 0 or the descriptors are NULL");
    if ((long long)first + count > db->p.capacity) return pl_fail(db, LL_ERR_CAPACITY, "places: upload: " + std::to_string(first) + " + " + std::to_string(count) + " places exceed the capacity " + std::to_string(db->p.capacity));
    if (count == 0) return LL_OK;
    PL_HIP(hipSetDevice(db->ctx->device));
    hipStream_t st = db->ctx->stream;
    PL_HIP(hipEventRecord(db->ev[0], st));
    PL_HIP(hipMemcpyAsync(db->d_desc + (size_t)first * PL_DESC, desc1200, (size_t)count * PL_DESC * sizeof(float), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pl_prepare, dim3((unsigned)count), dim3(64), 0, st, (const float *)db->d_desc, db->d_unit, db->d_mask, first);
    PL_HIP(hipEventRecord(db->ev[1], st));
    PL_HIP(hipGetLastError());
    db->add_pending = true; db->counts[0] = count;
    if (first + count > db->size) db->size = first + count;
    return LL_OK;
}

extern "C" int ll_places_download(ll_places *db, int first, int count, float *desc1200)
{
    if (!db) return LL_ERR_ARG;
    if (first < 0 || count < 0 || (long long)first + count > db->size || (count > 0 && !desc1200)) return pl_fail(db, LL_ERR_ARG, "places: download: range outside 0 .. size or the output is NULL");
    if (count == 0) return LL_OK;
    PL_HIP(hipSetDevice(db->ctx->device));
    PL_HIP(hipMemcpyAsync(desc1200, db->d_desc + (size_t)first * PL_DESC, (size_t)count * PL_DESC * sizeof(float), hipMemcpyDeviceToHost, db->ctx->stream));
    PL_HIP(hipStreamSynchronize(db->ctx->stream));
    return LL_OK;
}

/* the checks both calls share, then the [nq][nc] distances and shifts into the workspace (nq, nc >= 1) */
static int pl_check_ranges(ll_places *db, const char *who, int q0, int nq, int c0, int nc)
{
    if (q0 < 0 || nq < 0 || c0 < 0 || nc < 0 || (long long)q0 + nq > db->size || (long long)c0 + nc > db->size)
        return pl_fail(db, LL_ERR_ARG, std::string("places: ") + who + ": a range lies outside 0 .. size");
    if ((long long)nq * nc > PL_MAX_PAIRS) return pl_fail(db, LL_ERR_ARG, std::string("places: ") + who + ": nq * nc exceeds 2^26 pairs; split the call");
    return LL_OK;
}

static int pl_gram(ll_places *db, int q0, int nq, int c0, int nc)
{
    const size_t pairs = (size_t)nq * nc;
    if (!pl_grow(db->d_dist, db->cap_dist, pairs * sizeof(float)) || !pl_grow(db->d_shift, db->cap_shift, pairs))
        return pl_fail(db, LL_ERR_HIP, "places: hipMalloc failed for the distance workspace (" + std::to_string(pairs * 5) + " bytes)");
    const int nchunk = (nc + PL_CHUNK - 1) / PL_CHUNK;             /* nq * nchunk <= 2^26 / 64 + nq: one launch holds it */
    hipLaunchKernelGGL(k_pl_gram, dim3((unsigned)((size_t)nq * nchunk)), dim3(64 * PL_WAVES), 0, db->ctx->stream, (const float *)db->d_unit,
                       (const unsigned long long *)db->d_mask, q0, c0, nc, nchunk, db->d_dist, db->d_shift);
    return LL_OK;
}

extern "C" int ll_places_distances(ll_places *db, int q0, int nq, int c0, int nc, float *dist, unsigned char *shift)
{
    if (!db) return LL_ERR_ARG;
    int rc = pl_check_ranges(db, "distances", q0, nq, c0, nc); if (rc) return rc;
    if (nq > 0 && nc > 0 && (!dist || !shift)) return pl_fail(db, LL_ERR_ARG, "places: distances: an output is NULL");
    db->ms[1] = db->ms[2] = 0.0; db->counts[1] = (long long)nq * nc;
    if (nq == 0 || nc == 0) return LL_OK;
    PL_HIP(hipSetDevice(db->ctx->device));
    hipStream_t st = db->ctx->stream;
    const size_t pairs = (size_t)nq * nc;
    PL_HIP(hipEventRecord(db->ev[2], st));
    rc = pl_gram(db, q0, nq, c0, nc); if (rc) return rc;
    PL_HIP(hipEventRecord(db->ev[3], st));
    PL_HIP(hipGetLastError());
    PL_HIP(hipMemcpyAsync(dist, db->d_dist, pairs * sizeof(float), hipMemcpyDeviceToHost, st));
    PL_HIP(hipMemcpyAsync(shift, db->d_shift, pairs, hipMemcpyDeviceToHost, st));
    PL_HIP(hipStreamSynchronize(st));                              /* the ONE synchronisation */
    db->ms[1] = ll_event_ms(db->ev[2], db->ev[3], 0.0);
    return LL_OK;
}

extern "C" int ll_places_match(ll_places *db, int q0, int nq, int c0, int nc, const int *c_end, int K, int *id, float *dist, unsigned char *shift)
{
    if (!db) return LL_ERR_ARG;
    int rc = pl_check_ranges(db, "match", q0, nq, c0, nc); if (rc) return rc;
    if (K < 1 || K > PL_KMAX) return pl_fail(db, LL_ERR_ARG, "places: match: K outside 1 .. 8");
    if (nq > 0 && (!id || !dist || !shift)) return pl_fail(db, LL_ERR_ARG, "places: match: an output is NULL");
    db->ms[1] = db->ms[2] = 0.0; db->counts[1] = (long long)nq * nc;
    if (nq == 0) return LL_OK;
    const size_t n_out = (size_t)nq * K;
    if (nc == 0) {                                                 /* nothing to search: every rank is padding */
        for (size_t i = 0; i < n_out; ++i) { id[i] = -1; dist[i] = INFINITY; shift[i] = 0; }
        return LL_OK;
    }
    PL_HIP(hipSetDevice(db->ctx->device));
    hipStream_t st = db->ctx->stream;
    const size_t sel_bytes = n_out * 9;                            /* ids, distances, shifts */
    if (!pl_grow(db->d_sel, db->cap_sel, sel_bytes)) return pl_fail(db, LL_ERR_HIP, "places: hipMalloc failed for the results");
    if (c_end && !pl_grow(db->d_in, db->cap_in, (size_t)nq * sizeof(int))) return pl_fail(db, LL_ERR_HIP, "places: hipMalloc failed for c_end");
    unsigned char *pin = (unsigned char *)ll_pinned_scratch(sel_bytes);
    if (!pin) return pl_fail(db, LL_ERR_HIP, "places: no page-locked scratch");
    if (c_end) PL_HIP(hipMemcpyAsync(db->d_in, c_end, (size_t)nq * sizeof(int), hipMemcpyHostToDevice, st));
    int *d_id = (int *)db->d_sel; float *d_d = (float *)(db->d_sel + n_out * 4); unsigned char *d_s = db->d_sel + n_out * 8;
    PL_HIP(hipEventRecord(db->ev[2], st));
    rc = pl_gram(db, q0, nq, c0, nc); if (rc) return rc;
    PL_HIP(hipEventRecord(db->ev[3], st));
    hipLaunchKernelGGL(k_pl_select, dim3((unsigned)nq), dim3(256), 0, st, (const float *)db->d_dist, (const unsigned char *)db->d_shift, nc, c0,
                       c_end ? (const int *)db->d_in : nullptr, K, d_id, d_d, d_s);
    PL_HIP(hipEventRecord(db->ev[4], st));
    PL_HIP(hipGetLastError());
    PL_HIP(hipMemcpyAsync(pin, db->d_sel, sel_bytes, hipMemcpyDeviceToHost, st));
    PL_HIP(hipStreamSynchronize(st));                              /* the ONE synchronisation */
    std::memcpy(id, pin, n_out * 4); std::memcpy(dist, pin + n_out * 4, n_out * 4); std::memcpy(shift, pin + n_out * 8, n_out);
    db->ms[1] = ll_event_ms(db->ev[2], db->ev[3], 0.0); db->ms[2] = ll_event_ms(db->ev[3], db->ev[4], 0.0);
    return LL_OK;
}

/* ms3: describe + match-ready form of the last add / upload (this call waits for it), Gram matrices + diagonals and the selection
 * of the last distances / match; counts2: places of that add, pairs of that search */
extern "C" int ll_places_timing(ll_places *db, double *ms3, long long *counts2)
{
    if (!db) return LL_ERR_ARG;
    if (db->add_pending) {
        PL_HIP(hipSetDevice(db->ctx->device));
        PL_HIP(hipEventSynchronize(db->ev[1]));
        db->ms[0] = ll_event_ms(db->ev[0], db->ev[1], 0.0);
        db->add_pending = false;
    }
    if (ms3) for (int k = 0; k < 3; ++k) ms3[k] = db->ms[k];
    if (counts2) for (int k = 0; k < 2; ++k) counts2[k] = db->counts[k];
    return LL_OK;
}
