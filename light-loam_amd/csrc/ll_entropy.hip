/*
 * ll_entropy.hip -- ll_entropy: how crisp is the cloud that a list of stored keyframes makes under a list of poses?  Mean map entropy
 * (Droeschel, Stueckler & Behnke, ICRA 2014; Razlaw, Droeschel, Holz & Behnke, 2015) and mean plane variance from the covariance of
 * every point's fixed-radius neighbourhood, over the clouds of an ll_keyframes store; not in the reference, the contract is in
 * include/lightloam_hip.h.
 *
 * Every listed frame of a call has a list position k (counted across the ops) and every listed point a list index (the ops in order,
 * an op's frames in order, corner before surf); the host knows every size from the store's table and builds ONE table blob: the
 * (position, type) clouds where they lie in the pool with their first tiles, the poses [L][7], the ops' tile ranges.
 *   k_en_keys      a workgroup takes one 1024-point tile of one (frame, type) cloud: world point (ll_map_to_world), cell, 64-bit key
 *                  (op | cz | cy | cx, 17 bits a coordinate), the list index as value; a point without a cell gets the key ~0 and its
 *                  results (nn 0, NaN) at once;
 *   ll_sort_pairs  stable: list order survives inside a cell;
 *   k_en_heads / scan / k_en_cells   cell heads, their ranks, per cell its first sorted point and its key; the points gathered in
 *                  sorted order;
 *   k_en_rows      per occupied cell the nine (begin, end) ranges of sorted points -- the three x-adjacent cells of row (dz, dy) are
 *                  one contiguous range -- by binary search over the cell keys; dz, then dy ascending;
 *   k_en_moments   the hot kernel, below;
 *   k_en_tile_sums / k_en_op_sums   per tile a fixed tree, then an op's tiles in order.
 * Nothing atomic, every sum in a fixed order: a point's values and an op's record are the same bits alone, in any batch, at any op
 * position.
 *
 * THE CELL EDGE is 1.03125 * radius (f32 product), cx = floorf(x / cell) with the f32 quotient.  Why every neighbour under the f32 test
 * lies in the 27 cells around the query: let the x cells of p and q differ by two or more, say cx_p >= cx_q + 2.  The rounded quotient
 * is monotone and k + 2 and k + 1 are floats, so fl(px / cell) >= cx_q + 2 and fl(qx / cell) < cx_q + 1.  Both quotients are below
 * 2^16 in size in key range and carry at most half an ulp, 2^-8 together at that size (less near zero, where quotients are subnormal
 * only below 2^-126), so px - qx > cell * (1 - 2^-8) > 1.027 * radius.  The test's dx = fl(px - qx) > 1.027 * radius * (1 - 2^-24), and
 * d2 >= fl(dx * dx) rounded twice more (the other squares are >= 0, rounding is monotone), so d2 > 1.05 * radius^2 * (1 - 2^-22) >
 * fl(radius * radius): the pair fails the test.  The products must not be subnormal for the relative bounds: ll_entropy_create refuses
 * a radius whose f32 square is below 2^-100.  cell == radius would leave 2^-8 * radius of pairs that pass the test two cells apart.
 *
 * k_en_moments: ONE WAVE PER CELL (a workgroup of 64).  On the street scene of the tests a cell holds tens of points and its 27 cells
 * a few hundred: a 256-lane workgroup per cell would leave three waves of four without a query, or split the candidates between waves
 * and pay a cross-wave reduction of ten doubles per query in a fixed order; a wave needs neither, and a CU holds enough one-wave
 * workgroups to hide the global loads of the staging.  The nine row ranges are walked as ONE sequence in their order, staged through
 * LDS in chunks of EN_CHUNK float4 (a short row does not cost a barrier pair of its own); every lane reads candidate j at the same
 * address (a broadcast read), does the f32 test and, under its predicate, the ten f64 accumulations.  A cell of more than 64 points
 * walks the candidates once per 64 queries.  Then covariance, a fixed-sweep cyclic Jacobi, h and pv, stored at the query's list index.
 */
#include "ll_keyframes.h"
#include "ll_map_export.h"
#include "ll_map_search.h"
#include "ll_tiles.h"
#include <cmath>

#define EN_TILE 1024
#define EN_CHUNK 256                       /* float4 candidates per LDS staging chunk */
#define EN_SWEEPS 8                        /* cyclic Jacobi on a symmetric 3 x 3: converged to the last bit long before */
#define EN_BITS 17
#define EN_HALF 65536                      /* cells -65536 .. 65535 per axis */
#define EN_CELLS (1 << EN_BITS)
#define EN_MAX_OPS 1024
#define EN_SCAN_MAX (1 << 24)               /* ll_device_exscan takes 2^24 entries: a longer scan goes chunk by chunk, k_en_carry between them */
#define EN_MAX_POINTS (1ll << 27)          /* the sort's histogram scan (256 entries per 4096 keys) stays inside one ll_device_exscan */
#define EN_OUTSIDE (~0ull)
#define EN_LOG_2PIE3 8.513631199228036     /* 3 ln(2 pi e) */
#define EN_MASK ((unsigned long long)(EN_CELLS - 1))

struct EnSeg { long long off, base; int cnt; unsigned tile0; int k, op; };   /* off: first point in the pool; base: its list index; k: list position */
struct EnOpTiles { unsigned t0, t1; };
struct EnTile { double sum_h, sum_pv; long long pairs; int valid, sparse, outside, pad; };

struct ll_entropy : LLKfReader {
    ll_entropy_params p;
    unsigned char *d_mem = nullptr;               /* one allocation, carved at create from max_points */
    LLVoxWork W;                                  /* keys, values, flags, ranks and the sort's and the scan's scratch */
    float4 *d_world = nullptr, *d_spts = nullptr; /* world points by list index, and in sorted order */
    float *d_h = nullptr, *d_pv = nullptr; int *d_nn = nullptr;   /* by list index; nn unsaturated */
    int *d_cs = nullptr; unsigned long long *d_ck = nullptr; int2 *d_rows = nullptr;
    EnTile *d_tile = nullptr; ll_entropy_rec *d_rec = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<long long> last_base; std::vector<int> last_n0, last_n1;   /* the last run's listed frames by list position */
    double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};     /* the last run: keys, sort + cells, rows, moments, sums (events) */
    long long counts[5] = {0, 0, 0, 0, 0};        /* listed frames, their points, occupied cells, neighbour pairs, host synchronisations */
};

__device__ __forceinline__ unsigned long long en_key(int op, int cz, int cy, int cx)
{
    return ((unsigned long long)op << (3 * EN_BITS)) | ((unsigned long long)cz << (2 * EN_BITS)) | ((unsigned long long)cy << EN_BITS) | (unsigned long long)cx;
}

/* the cell coordinate of x shifted to 0 .. 2^17 - 1; -1: none (not finite, or beyond the key range) */
__device__ __forceinline__ int en_cell(float x, float cell)
{
    const float f = floorf(x / cell);
    if (!(f >= (float)-EN_HALF && f < (float)EN_HALF)) return -1;
    return (int)f + EN_HALF;
}

__global__ __launch_bounds__(256) void k_en_keys(const float4 *__restrict__ pool, const EnSeg *__restrict__ seg, int nseg, const double *__restrict__ poses,
                                                 float cell, float4 *world, unsigned long long *keys, int *vals, float *h, float *pv, int *nn)
{
    const EnSeg s = seg[ll_tile_find(seg, nseg, blockIdx.x)];
    const int first = (int)(blockIdx.x - s.tile0) * EN_TILE, n = min(EN_TILE, s.cnt - first);
    const float4 *src = pool + s.off + first;
    const int k = __builtin_amdgcn_readfirstlane(s.k), op = __builtin_amdgcn_readfirstlane(s.op);
    double P[7];
    for (int j = 0; j < 7; ++j) P[j] = poses[(size_t)k * 7 + j];
    float4 po[EN_TILE / 256];
#pragma unroll
    for (int j = 0; j < EN_TILE / 256; ++j) po[j] = src[min(j * 256 + (int)threadIdx.x, n - 1)];
#pragma unroll
    for (int j = 0; j < EN_TILE / 256; ++j) {
        const int i = j * 256 + (int)threadIdx.x;
        if (i >= n) continue;
        float wx, wy, wz;
        ll_map_to_world(P, po[j], wx, wy, wz);
        const int cx = en_cell(wx, cell), cy = en_cell(wy, cell), cz = en_cell(wz, cell);
        const bool in = cx >= 0 && cy >= 0 && cz >= 0;
        const long long idx = s.base + first + i;
        world[idx] = make_float4(wx, wy, wz, 0.0f);
        vals[idx] = (int)idx;
        keys[idx] = in ? en_key(op, cz, cy, cx) : EN_OUTSIDE;
        if (!in) { h[idx] = __builtin_nanf(""); pv[idx] = __builtin_nanf(""); nn[idx] = 0; }
    }
}

/* the points without a cell are one run at the end of the sorted keys: it counts as one more "cell", which k_en_moments skips */
__global__ __launch_bounds__(256) void k_en_heads(const unsigned long long *__restrict__ keys, const int *__restrict__ vals, const float4 *__restrict__ world, int n,
                                                  int *flag, float4 *spts)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
    spts[i] = world[vals[i]];
}

/* a chunk of the scan after the first: what stood before it -- the last entry of the chunk before, already final, and that entry's flag */
__global__ __launch_bounds__(256) void k_en_carry(int *rank, int len, const int *prev_rank, const int *prev_flag)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i < len) rank[i] += *prev_rank + *prev_flag;
}

/* rank: the exclusive scan of flag over n + 1 entries, rank[n] = the number of cells */
__global__ __launch_bounds__(256) void k_en_cells(const unsigned long long *__restrict__ keys, const int *__restrict__ flag, const int *__restrict__ rank, int n,
                                                  int *cs, unsigned long long *ck)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    if (flag[i]) { cs[rank[i]] = i; ck[rank[i]] = keys[i]; }
    if (i == n - 1) cs[rank[n]] = n;
}

/* one thread per (cell, row): the sorted points of cells (cx - 1 .. cx + 1, cy + dy, cz + dz) of the cell's op */
__global__ __launch_bounds__(256) void k_en_rows(const unsigned long long *__restrict__ ck, const int *__restrict__ cs, int ncell, int2 *rows)
{
    const int t = blockIdx.x * 256 + (int)threadIdx.x;
    if (t >= ncell * 9) return;
    const int c = t / 9, r = t - c * 9;
    const unsigned long long key = ck[c];
    int2 out = make_int2(0, 0);
    const int cx = (int)(key & EN_MASK), cy = (int)((key >> EN_BITS) & EN_MASK) + (r % 3 - 1), cz = (int)((key >> (2 * EN_BITS)) & EN_MASK) + (r / 3 - 1);
    if (key != EN_OUTSIDE && cy >= 0 && cy < EN_CELLS && cz >= 0 && cz < EN_CELLS) {
        const int op = (int)(key >> (3 * EN_BITS));
        const unsigned long long klo = en_key(op, cz, cy, max(cx - 1, 0)), khi = en_key(op, cz, cy, min(cx + 1, EN_CELLS - 1));
        int lo = 0, hi = ncell;                                     /* the first cell with a key >= klo */
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (ck[mid] < klo) lo = mid + 1; else hi = mid; }
        const int a = lo;
        hi = ncell;                                                  /* the first cell with a key > khi, from a on */
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (ck[mid] <= khi) lo = mid + 1; else hi = mid; }
        out = make_int2(cs[a], cs[lo]);
    }
    rows[t] = out;
}

/* the eigenvalues of the symmetric a [3][3] (destroyed), ascending: ll_info_eig's rotation on a 3 x 3, every sweep visits (0,1) (0,2)
 * (1,2), a pair whose off-diagonal entry is exactly 0 is left alone; no data-dependent iteration count */
__device__ __forceinline__ void en_eig3(double (&a)[9], double eig[3])
{
#pragma unroll 1
    for (int sweep = 0; sweep < EN_SWEEPS; ++sweep)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p * 3 + q];
                if (apq == 0.0) continue;
                const double theta = (a[q * 3 + q] - a[p * 3 + p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double akp = a[k * 3 + p], akq = a[k * 3 + q];
                    a[k * 3 + p] = c * akp - s * akq; a[k * 3 + q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double apk = a[p * 3 + k], aqk = a[q * 3 + k];
                    a[p * 3 + k] = c * apk - s * aqk; a[q * 3 + k] = s * apk + c * aqk;
                }
            }
#pragma unroll
    for (int k = 0; k < 3; ++k) eig[k] = a[k * 4];
#pragma unroll
    for (int i = 1; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3 - i; ++k) {
            const double lo = eig[k] <= eig[k + 1] ? eig[k] : eig[k + 1], hi = eig[k] <= eig[k + 1] ? eig[k + 1] : eig[k];
            eig[k] = lo; eig[k + 1] = hi;
        }
}

__global__ __launch_bounds__(64) void k_en_moments(const float4 *__restrict__ spts, const int *__restrict__ vals, const int *__restrict__ cs,
                                                   const unsigned long long *__restrict__ ck, const int2 *__restrict__ rows, float r2, int min_nb,
                                                   double lfloor, float *h, float *pv, int *nn)
{
    const int c = blockIdx.x, lane = (int)threadIdx.x;
    if (ck[c] == EN_OUTSIDE) return;                                /* the same for the whole workgroup */
    __shared__ float4 stage[EN_CHUNK];
    const int q0 = __builtin_amdgcn_readfirstlane(cs[c]), q1 = __builtin_amdgcn_readfirstlane(cs[c + 1]);
    int rb[9], rl[9], total = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int2 v = rows[(size_t)c * 9 + r];
        rb[r] = __builtin_amdgcn_readfirstlane(v.x); rl[r] = __builtin_amdgcn_readfirstlane(v.y) - rb[r];
        total += rl[r];
    }
    for (int qb = q0; qb < q1; qb += 64) {
        const bool live = qb + lane < q1;
        const int qi = live ? qb + lane : q1 - 1;
        const float4 q = spts[qi];
        int cnt = 0;
        double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
        for (int t0 = 0; t0 < total; t0 += EN_CHUNK) {
            const int m = min(EN_CHUNK, total - t0);
            __syncthreads();                                        /* the chunk before has been read by every lane */
#pragma unroll
            for (int k = 0; k < EN_CHUNK / 64; ++k) {
                const int t = k * 64 + lane;
                if (t >= m) continue;
                int s = t0 + t, src = 0; bool found = false;        /* entry s of the nine ranges laid end to end */
#pragma unroll
                for (int r = 0; r < 9; ++r) {
                    if (!found && s < rl[r]) { src = rb[r] + s; found = true; }
                    if (!found) s -= rl[r];
                }
                stage[t] = spts[src];
            }
            __syncthreads();
            for (int j = 0; j < m; ++j) {
                const float4 p = stage[j];                          /* one address for the wave: a broadcast read */
                const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 <= r2) {
                    const double ex = (double)dx, ey = (double)dy, ez = (double)dz;
                    ++cnt;
                    sx += ex; sy += ey; sz += ez;
                    sxx += ex * ex; sxy += ex * ey; sxz += ex * ez; syy += ey * ey; syz += ey * ez; szz += ez * ez;
                }
            }
        }
        /* Sigma = S2 / n - (S1 / n)(S1 / n)^T; n >= 1: the query is its own neighbour */
        const double dn = (double)cnt;
        const double mx = sx / dn, my = sy / dn, mz = sz / dn;
        double a[9], eig[3];
        a[0] = sxx / dn - mx * mx; a[1] = sxy / dn - mx * my; a[2] = sxz / dn - mx * mz;
        a[4] = syy / dn - my * my; a[5] = syz / dn - my * mz; a[8] = szz / dn - mz * mz;
        a[3] = a[1]; a[6] = a[2]; a[7] = a[5];
        en_eig3(a, eig);
        float oh = __builtin_nanf(""), opv = __builtin_nanf("");
        if (cnt >= min_nb) {
            opv = (float)fmax(eig[0], 0.0);
            oh = (float)(0.5 * (EN_LOG_2PIE3 + ((log(fmax(eig[0], lfloor)) + log(fmax(eig[1], lfloor))) + log(fmax(eig[2], lfloor)))));
        }
        if (live) {
            const int idx = vals[qi];
            nn[idx] = cnt; h[idx] = oh; pv[idx] = opv;
        }
    }
}

/* a tile's partial: thread t adds its points t, t + 256, t + 512, t + 768 in that order, then the 256 partials fold by halves
 * (t += t + 128, t += t + 64, ..).  Only valid points have addends; the others count */
__global__ __launch_bounds__(256) void k_en_tile_sums(const EnSeg *__restrict__ seg, int nseg, const float *__restrict__ h, const float *__restrict__ pv,
                                                      const int *__restrict__ nn, int min_nb, EnTile *tiles)
{
    const EnSeg s = seg[ll_tile_find(seg, nseg, blockIdx.x)];
    const int first = (int)(blockIdx.x - s.tile0) * EN_TILE, n = min(EN_TILE, s.cnt - first), tid = (int)threadIdx.x;
    const long long base = s.base + first;
    __shared__ double sh[256], sp[256];
    __shared__ long long spairs[256];
    __shared__ int sc[3][256];
    double ah = 0.0, ap = 0.0; long long pairs = 0; int nv = 0, ns = 0, no = 0;
#pragma unroll
    for (int j = 0; j < EN_TILE / 256; ++j) {
        const int i = j * 256 + tid;
        if (i >= n) continue;
        const int c = nn[base + i];
        if (c == 0) { ++no; continue; }
        pairs += c;
        if (c < min_nb) { ++ns; continue; }
        ++nv; ah += (double)h[base + i]; ap += (double)pv[base + i];
    }
    sh[tid] = ah; sp[tid] = ap; spairs[tid] = pairs; sc[0][tid] = nv; sc[1][tid] = ns; sc[2][tid] = no;
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) {
            sh[tid] += sh[tid + o]; sp[tid] += sp[tid + o]; spairs[tid] += spairs[tid + o];
            sc[0][tid] += sc[0][tid + o]; sc[1][tid] += sc[1][tid + o]; sc[2][tid] += sc[2][tid + o];
        }
    }
    if (tid == 0) { EnTile T = {sh[0], sp[0], spairs[0], sc[0][0], sc[1][0], sc[2][0], 0}; tiles[blockIdx.x] = T; }
}

/* a workgroup of 64 per op: its tiles in order, from zero; 64 partials are fetched at a time, lane 0 adds them */
__global__ __launch_bounds__(64) void k_en_op_sums(const EnOpTiles *__restrict__ ops, const EnTile *__restrict__ tiles, ll_entropy_rec *rec)
{
    const EnOpTiles o = ops[blockIdx.x];
    __shared__ EnTile buf[64];
    ll_entropy_rec R = {0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0};
    for (unsigned t0 = o.t0; t0 < o.t1; t0 += 64) {
        const int m = (int)min(64u, o.t1 - t0);
        __syncthreads();
        if ((int)threadIdx.x < m) buf[threadIdx.x] = tiles[t0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int j = 0; j < m; ++j) {
                R.n_valid += buf[j].valid; R.n_sparse += buf[j].sparse; R.n_outside += buf[j].outside; R.n_pairs += buf[j].pairs;
                R.sum_h += buf[j].sum_h; R.sum_pv += buf[j].sum_pv;
            }
    }
    if (threadIdx.x == 0) {
        R.n_points = R.n_valid + R.n_sparse + R.n_outside;
        if (R.n_valid > 0) { R.mme = R.sum_h / (double)R.n_valid; R.mpv = R.sum_pv / (double)R.n_valid; }
        rec[blockIdx.x] = R;
    }
}

/* ------------------------------------------------------------------ host side */
#define EN_HIP(call) LL_HIP_CHECK(ll_fail, v, "entropy: ", call, #call)

extern "C" void ll_entropy_default_params(ll_entropy_params *p)
{
    if (!p) return;
    p->radius = 0.5f; p->min_neighbours = 6; p->lambda_floor = 1e-6f; p->max_points = 1 << 20;
}

/* the parts of the one allocation behind the sort's workspace; base == nullptr: the size only */
static size_t en_carve(ll_entropy *v, unsigned char *base, size_t cap)
{
    LLCarve C{base};
    v->d_world = C.take<float4>(cap); v->d_spts = C.take<float4>(cap);
    v->d_h = C.take<float>(cap); v->d_pv = C.take<float>(cap); v->d_nn = C.take<int>(cap);
    v->d_cs = C.take<int>(cap + 1); v->d_ck = C.take<unsigned long long>(cap); v->d_rows = C.take<int2>(cap * 9);
    v->d_tile = C.take<EnTile>(cap);                                /* a tile holds at least one point */
    v->d_rec = C.take<ll_entropy_rec>(EN_MAX_OPS);
    return C.at;
}

extern "C" int ll_entropy_create(ll_keyframes *kf, const ll_entropy_params *p, ll_entropy **out)
{
    if (!kf || !p || !out) return LL_ERR_ARG;
    *out = nullptr;
    if (!(p->radius > 0.0f) || !(p->radius <= 8.0f) || !(p->radius * p->radius >= 0x1p-100f) || p->min_neighbours < 4 || !(p->lambda_floor > 0.0f) ||
        !std::isfinite(p->lambda_floor) || p->max_points < 1 || p->max_points > EN_MAX_POINTS)
        return llkf_create_err(kf, LL_ERR_ARG, "entropy: bad parameters (radius in (0, 8] with a square of at least 2^-100, min_neighbours >= 4, lambda_floor > 0 and finite, "
                                         "max_points in 1 .. 2^27)");
    ll_ctx *ctx = kf->ctx;
    if (hipSetDevice(ctx->device) != hipSuccess) return llkf_create_err(kf, LL_ERR_HIP, "entropy: hipSetDevice failed");
    ll_entropy *v = new ll_entropy();
    v->follow(kf); v->p = *p;
    const size_t cap = (size_t)p->max_points;
    const size_t own = en_carve(v, nullptr, cap), bytes = own + ll_vox_work_bytes((int)cap, 1);
    bool ok = hipMalloc((void **)&v->d_mem, bytes) == hipSuccess;
    for (int k = 0; ok && k < 6; ++k) ok = hipEventCreate(&v->ev[k]) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ll_entropy_destroy(v);
        return llkf_create_err(kf, LL_ERR_HIP, "entropy: no device memory for " + std::to_string(bytes) + " bytes of workspace");
    }
    en_carve(v, v->d_mem, cap);
    ll_vox_work_carve(v->d_mem + own, (int)cap, 1, &v->W);
    *out = v;
    return LL_OK;
}

extern "C" void ll_entropy_destroy(ll_entropy *v)
{
    if (!v) return;
    v->release();
    if (v->d_mem) (void)hipFree(v->d_mem);
    for (int k = 0; k < 6; ++k) if (v->ev[k]) (void)hipEventDestroy(v->ev[k]);
    delete v;
}

extern "C" const char *ll_entropy_last_error(const ll_entropy *v) { return v ? v->err.c_str() : "null entropy"; }

static int en_stale(ll_entropy *v) { return v->stale("entropy: the store was reset since the object followed it: call ll_entropy_reset"); }

extern "C" int ll_entropy_reset(ll_entropy *v)
{
    if (!v) return LL_ERR_ARG;
    v->epoch = v->kf->n_reset;
    v->last_base.clear(); v->last_n0.clear(); v->last_n1.clear();
    for (int k = 0; k < 5; ++k) { v->ms[k] = 0.0; v->counts[k] = 0; }
    return LL_OK;
}

extern "C" int ll_entropy_run(ll_entropy *v, const ll_entropy_op *ops, int n_ops, ll_entropy_rec *rec)
{
    if (!v) return LL_ERR_ARG;
    if (!ops || n_ops < 1 || !rec) return v->fail(LL_ERR_ARG, "entropy: ops or rec is NULL or n_ops < 1");
    if (n_ops > EN_MAX_OPS) return v->fail(LL_ERR_CAPACITY, "entropy: " + std::to_string(n_ops) + " ops, one call takes at most " + std::to_string(EN_MAX_OPS));
    const ll_keyframes *kf = v->kf;
    const ll_keyframe_info *tab = kf->tab.data();
    const int size = (int)kf->tab.size();
    /* ---- every refusal before anything is enqueued or a value changes */
    long long L = 0, n_points = 0;
    std::vector<int> seen(size, -1);                                /* the last op that listed the frame */
    for (int i = 0; i < n_ops; ++i) {
        const ll_entropy_op &o = ops[i];
        const std::string who = "entropy: op " + std::to_string(i) + ": ";
        if (o.n_frames < 0 || (o.n_frames > 0 && !o.frames)) return v->fail(LL_ERR_ARG, who + "n_frames < 0 or frames is NULL");
        long long pts;
        if (llkf_check(tab, size, {o.n_frames, o.frames, o.poses_w7, ""}, LLKF_DUP_PER_OP, &seen, i, who, &v->err, &pts)) return LL_ERR_ARG;
        n_points += pts;
        L += o.n_frames;
    }
    if (n_points > v->p.max_points) return v->fail(LL_ERR_CAPACITY, "entropy: " + std::to_string(n_points) + " listed points, max_points is " + std::to_string(v->p.max_points));
    int rc = en_stale(v); if (rc) return rc;
    /* ---- the tables: clouds, poses, the ops' tiles */
    std::vector<EnSeg> segs;
    std::vector<double> poses((size_t)L * 7);
    std::vector<EnOpTiles> optab((size_t)n_ops);
    std::vector<long long> base((size_t)L); std::vector<int> n0((size_t)L), n1((size_t)L);
    LLTiler tiles{EN_TILE};
    long long at = 0; int k0 = 0;
    for (int i = 0; i < n_ops; ++i) {
        const ll_entropy_op &o = ops[i];
        optab[i].t0 = (unsigned)tiles.next;
        const LLKfList list = {o.n_frames, o.frames, o.poses_w7, ""};
        for (int f = 0; f < o.n_frames; ++f) {
            const double *P = llkf_pose(tab, list, f);
            for (int k = 0; k < 7; ++k) poses[(size_t)(k0 + f) * 7 + k] = P[k];
            base[k0 + f] = at; n0[k0 + f] = tab[o.frames[f]].n[0]; n1[k0 + f] = tab[o.frames[f]].n[1];
            for (int w = 0; w < 2; ++w) {
                const LLKfCloud c = llkf_cloud(tab, kf->cap[0], o.frames[f], w);
                if (c.cnt <= 0) continue;
                segs.push_back({c.off, at, c.cnt, tiles.take(c.cnt), k0 + f, i});
                at += c.cnt;
            }
        }
        optab[i].t1 = (unsigned)tiles.next;
        k0 += o.n_frames;
    }
    v->last_base = base; v->last_n0 = n0; v->last_n1 = n1;
    for (int k = 0; k < 5; ++k) { v->ms[k] = 0.0; v->counts[k] = 0; }
    v->counts[0] = L; v->counts[1] = n_points;
    const int n = (int)n_points;
    if (n == 0) {
        for (int i = 0; i < n_ops; ++i) { const ll_entropy_rec Z = {0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0}; rec[i] = Z; }
        return LL_OK;
    }
    std::vector<unsigned char> blob;
    const size_t at_seg = ll_blob_put(blob, segs), at_pose = ll_blob_put(blob, poses), at_op = ll_blob_put(blob, optab);
    hipStream_t st = v->ctx->stream;
    EN_HIP(hipSetDevice(v->ctx->device));
    ll_entropy_rec *pin = (ll_entropy_rec *)ll_pinned_scratch((size_t)n_ops * sizeof(ll_entropy_rec) + sizeof(int));
    if (!pin) return v->fail(LL_ERR_HIP, "entropy: no page-locked scratch");
    const unsigned char *d_blob = (const unsigned char *)llx_stage_bytes(v->X, blob.data(), blob.size(), st, v->err);
    if (!d_blob) return LL_ERR_HIP;
    const EnSeg *d_seg = (const EnSeg *)(d_blob + at_seg);
    const LLVoxWork &W = v->W;
    const float cell = v->p.radius * 1.03125f, r2 = v->p.radius * v->p.radius;
    const unsigned nt = (unsigned)tiles.next, nb = (unsigned)((n + 255) / 256);
    long long syncs = 0;
    EN_HIP(hipEventRecord(v->ev[0], st));
    hipLaunchKernelGGL(k_en_keys, dim3(nt), dim3(256), 0, st, (const float4 *)kf->pool, d_seg, (int)segs.size(), (const double *)(d_blob + at_pose), cell, v->d_world,
                       W.keys, W.vals, v->d_h, v->d_pv, v->d_nn);
    EN_HIP(hipEventRecord(v->ev[1], st));
    if (ll_sort_pairs_reads_back(n)) ++syncs;
    if (ll_sort_pairs(W.keys, W.vals, W.tmp_keys, W.tmp_vals, n, W.hist, W.tile_sum, W.or_and, st)) return v->fail(LL_ERR_HIP, "entropy: the sort's read-back failed");
    hipLaunchKernelGGL(k_en_heads, dim3(nb), dim3(256), 0, st, (const unsigned long long *)W.keys, (const int *)W.vals, (const float4 *)v->d_world, n, W.flag, v->d_spts);
    ll_copy_d2d(W.rank, W.flag, (size_t)n * sizeof(int), st);
    ll_fill_words(W.rank + n, 1, 0, 0, 1, st);
    for (long long c0 = 0; c0 < (long long)n + 1; c0 += EN_SCAN_MAX) {   /* rank[n] = the number of cells */
        const int len = (int)std::min<long long>(EN_SCAN_MAX, (long long)n + 1 - c0);
        ll_device_exscan(W.rank + c0, len, W.tile_sum, st);
        if (c0) hipLaunchKernelGGL(k_en_carry, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, W.rank + c0, len, (const int *)(W.rank + c0 - 1), (const int *)(W.flag + c0 - 1));
    }
    hipLaunchKernelGGL(k_en_cells, dim3(nb), dim3(256), 0, st, (const unsigned long long *)W.keys, (const int *)W.flag, (const int *)W.rank, n, v->d_cs, v->d_ck);
    EN_HIP(hipEventRecord(v->ev[2], st));
    int *pin_cells = (int *)(pin + n_ops);
    EN_HIP(hipMemcpyAsync(pin_cells, W.rank + n, sizeof(int), hipMemcpyDeviceToHost, st));
    EN_HIP(hipStreamSynchronize(st)); ++syncs;                       /* the one read that sizes the two launches per cell */
    const int ncell = *pin_cells;
    if (ncell < 1 || ncell > n) return v->fail(LL_ERR_HIP, "entropy: " + std::to_string(ncell) + " cells for " + std::to_string(n) + " points");
    hipLaunchKernelGGL(k_en_rows, dim3((unsigned)(((long long)ncell * 9 + 255) / 256)), dim3(256), 0, st, (const unsigned long long *)v->d_ck, (const int *)v->d_cs, ncell, v->d_rows);
    EN_HIP(hipEventRecord(v->ev[3], st));
    hipLaunchKernelGGL(k_en_moments, dim3((unsigned)ncell), dim3(64), 0, st, (const float4 *)v->d_spts, (const int *)W.vals, (const int *)v->d_cs,
                       (const unsigned long long *)v->d_ck, (const int2 *)v->d_rows, r2, v->p.min_neighbours, (double)v->p.lambda_floor, v->d_h, v->d_pv, v->d_nn);
    EN_HIP(hipEventRecord(v->ev[4], st));
    hipLaunchKernelGGL(k_en_tile_sums, dim3(nt), dim3(256), 0, st, d_seg, (int)segs.size(), (const float *)v->d_h, (const float *)v->d_pv, (const int *)v->d_nn,
                       v->p.min_neighbours, v->d_tile);
    hipLaunchKernelGGL(k_en_op_sums, dim3((unsigned)n_ops), dim3(64), 0, st, (const EnOpTiles *)(d_blob + at_op), (const EnTile *)v->d_tile, v->d_rec);
    EN_HIP(hipEventRecord(v->ev[5], st));
    EN_HIP(hipMemcpyAsync(pin, v->d_rec, (size_t)n_ops * sizeof(ll_entropy_rec), hipMemcpyDeviceToHost, st));
    EN_HIP(hipGetLastError());
    EN_HIP(hipStreamSynchronize(st)); ++syncs;
    std::memcpy(rec, pin, (size_t)n_ops * sizeof(ll_entropy_rec));
    for (int k = 0; k < 5; ++k) v->ms[k] = ll_event_ms(v->ev[k], v->ev[k + 1], 0.0);
    long long outside = 0, pairs = 0;
    for (int i = 0; i < n_ops; ++i) { outside += rec[i].n_outside; pairs += rec[i].n_pairs; }
    v->counts[2] = ncell - (outside > 0 ? 1 : 0); v->counts[3] = pairs; v->counts[4] = syncs;
    return LL_OK;
}

extern "C" int ll_entropy_values(ll_entropy *v, int k, float *h, float *pv, unsigned short *nn)
{
    if (!v) return LL_ERR_ARG;
    int rc = en_stale(v); if (rc) return rc;
    if (k < 0 || k >= (int)v->last_base.size()) return v->fail(LL_ERR_ARG, "entropy: the last run listed " + std::to_string(v->last_base.size()) + " frames, there is no frame " + std::to_string(k));
    const size_t n = (size_t)v->last_n0[k] + (size_t)v->last_n1[k];
    if (n == 0 || (!h && !pv && !nn)) return LL_OK;
    const long long b = v->last_base[k];
    const LLKfRange ranges[3] = {{h ? v->d_h + b : nullptr, n * 4, h}, {pv ? v->d_pv + b : nullptr, n * 4, pv}, {nn ? v->d_nn + b : nullptr, n * 4, nullptr}};
    const unsigned char *pin;
    rc = v->read("entropy: ", ranges, 3, &pin); if (rc) return rc;
    if (nn) { const int *c = (const int *)(pin + n * 8); for (size_t i = 0; i < n; ++i) nn[i] = (unsigned short)(c[i] > 65535 ? 65535 : c[i]); }
    return LL_OK;
}

extern "C" int ll_entropy_timing(const ll_entropy *v, double *ms, long long *counts)
{
    return v ? llkf_timing(v->ms, v->counts, 5, ms, counts) : LL_ERR_ARG;
}
