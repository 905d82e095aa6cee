/*
 * ll_pcm.hip -- ll_pcm: pairwise-consistent sets of loop-closure candidates (Mangelson et al., "Pairwise Consistent Measurement Set
 * Maximization", ICRA 2018, in the threshold form of Kimera-RPGO's PcmSimple).  Not in the reference; the contract, float by float, is
 * in include/lightloam_hip.h, the pair arithmetic in ll_pcm_math.h (shared with ll_pcm_host).
 *
 * A call holds n_graphs ragged graphs; a graph's C <= 4096 candidates make a C x C bit matrix of W = ceil(C / 64) words a row, the
 * graphs' matrices back to back.  After the first two kernels everything is integer.
 *   k_pcm_prepare    a thread per candidate: B, Ai, P_i, s_i, s_j (PCM_PREP doubles);
 *   k_pcm_adjacency  a workgroup takes 256 rows of ONE word: the word's 64 column candidates are staged in LDS and read at one address
 *                    by every lane (a broadcast), a thread owns a row and keeps its candidate in registers.  The pair is always
 *                    evaluated as (min, max), so both triangles come from the same arithmetic: no transpose, no atomic.  One 8-byte
 *                    store per thread;
 *   k_pcm_degree     a wave per row: popcounts, a wave sum.  Also the first stage of ll_pcm_select, whose matrices come from the caller;
 *   k_pcm_rank       rank[c] = the candidates before c by (degree descending, index ascending), degrees staged in LDS; order = its inverse;
 *   k_pcm_relabel    the matrix in rank order, rows and columns: "earliest in the order" becomes find-first-set.  A wave per row, the
 *                    row and the order in LDS, lane l gathers the 64 bits of its word along a diagonal (bank (k + l) % 64);
 *   k_pcm_clique     ONE WAVE PER START: lane l holds word l of U.  A step is a ballot of the non-zero words, ctz in the lowest such
 *                    lane, a broadcast, and one coalesced read of a row (at most 512 bytes, L2-resident).  No LDS, no barrier.  A start
 *                    whose degree + 1, with its index, cannot beat a (size, start) some wave has already published is skipped: an
 *                    integer atomicMax on a packed key, which changes work, never the result;
 *   k_pcm_pick       per graph the largest size, ties to the earliest start; its clique walked once more (the walk is deterministic) to
 *                    write membership in original order, and the record.
 * Seven launches and one small clear whatever the number of graphs, one upload, ONE host synchronisation.  No floating-point atomic.
 */
#include "ll_internal.h"
#include "ll_pcm_math.h"
#include <algorithm>
#include <cmath>

#define PCM_ROWS 256                                /* rows per k_pcm_adjacency workgroup */
#define PCM_KEY_BITS 12

struct PcmGraph { long long woff; int c0, C, W, pad; };             /* woff: the matrix's first word; c0: the first candidate */
struct PcmCand { double Z[7]; int i, j; };                         /* i, j: rows of the call's pose table */

struct ll_pcm {
    ll_ctx *ctx = nullptr;
    int max_graphs = 0, max_nodes = 0, max_cands = 0;
    unsigned char *d_mem = nullptr;                 /* create-time: the upload's room and everything per candidate / per graph */
    size_t up_bytes = 0;
    unsigned char *d_up = nullptr;
    double *d_prep = nullptr;
    int *d_deg = nullptr, *d_rank = nullptr, *d_order = nullptr, *d_size = nullptr;
    unsigned char *d_sel = nullptr;
    ll_pcm_record *d_rec = nullptr;
    unsigned long long *d_steps = nullptr; unsigned *d_best = nullptr;   /* per graph, cleared per call (d_best directly behind d_steps) */
    unsigned long long *d_words = nullptr;          /* [2][words_cap]: original order, rank order; allocated at the first call, grown on demand */
    size_t words_cap = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<PcmGraph> last;                     /* the last run's or select's graphs */
    bool has_run = false;
    double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};       /* prepare, adjacency, order (degree + rank + relabel), clique, pick */
    long long counts[4] = {0, 0, 0, 0};             /* graphs, candidates, pairs evaluated, clique steps */
    std::string err;
};

/* ------------------------------------------------------------------ device */
__global__ __launch_bounds__(256) void k_pcm_prepare(const double *__restrict__ poses, const double *__restrict__ s, const PcmCand *__restrict__ cand, int n, double *prep)
{
    const int c = blockIdx.x * 256 + (int)threadIdx.x;
    if (c >= n) return;
    const PcmCand k = cand[c];
    double Pi[7], Pj[7], out[PCM_PREP];
    for (int m = 0; m < 7; ++m) { Pi[m] = poses[(size_t)k.i * 7 + m]; Pj[m] = poses[(size_t)k.j * 7 + m]; }
    pcm_prepare(Pi, Pj, k.Z, s[k.i], s[k.j], out);
    for (int m = 0; m < PCM_PREP; ++m) prep[(size_t)c * PCM_PREP + m] = out[m];
}

/* blockIdx.y: the graph; blockIdx.x = row block * W + word */
__global__ __launch_bounds__(PCM_ROWS) void k_pcm_adjacency(const PcmGraph *__restrict__ graphs, const double *__restrict__ prep, PcmTol tol, unsigned long long *words)
{
    const PcmGraph G = graphs[blockIdx.y];
    if (G.W == 0) return;
    const int rb = (int)blockIdx.x / G.W, w = (int)blockIdx.x - rb * G.W;
    if (rb * PCM_ROWS >= G.C) return;                               /* the same for the whole workgroup, before the barrier */
    __shared__ double col[64 * PCM_PREP];
    const int ncol = min(64, G.C - w * 64);
    const double *src = prep + ((size_t)G.c0 + (size_t)w * 64) * PCM_PREP;
    for (int k = (int)threadIdx.x; k < ncol * PCM_PREP; k += PCM_ROWS) col[k] = src[k];
    __syncthreads();
    const int r = rb * PCM_ROWS + (int)threadIdx.x;
    if (r >= G.C) return;
    double row[PCM_PREP];
    const double *rsrc = prep + ((size_t)G.c0 + r) * PCM_PREP;
#pragma unroll
    for (int k = 0; k < PCM_PREP; ++k) row[k] = rsrc[k];
    unsigned long long bits = 0;
    for (int k = 0; k < ncol; ++k) {
        const int d = w * 64 + k;
        const double *o = col + k * PCM_PREP;                       /* one address for the wave: a broadcast read */
        bool ok = false;
        if (r < d) ok = pcm_pair(row, row + 14, row[21], row[22], o + 7, o[21], o[22], tol);
        else if (r > d) ok = pcm_pair(o, o + 14, o[21], o[22], row + 7, row[21], row[22], tol);
        if (ok) bits |= 1ull << k;
    }
    words[G.woff + (size_t)r * G.W + w] = bits;
}

/* a wave per row; grid (ceil(max C / 4), graphs) */
__global__ __launch_bounds__(256) void k_pcm_degree(const PcmGraph *__restrict__ graphs, const unsigned long long *__restrict__ words, int *deg)
{
    const PcmGraph G = graphs[blockIdx.y];
    const int lane = (int)threadIdx.x & 63, r = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + ((int)threadIdx.x >> 6));
    if (r >= G.C) return;
    const int n = lane < G.W ? __popcll(words[G.woff + (size_t)r * G.W + lane]) : 0;
    const int sum = ll_wave_sum_i32(n);
    if (lane == 0) deg[G.c0 + r] = sum;
}

/* grid (ceil(max C / 256), graphs) */
__global__ __launch_bounds__(256) void k_pcm_rank(const PcmGraph *__restrict__ graphs, const int *__restrict__ deg, int *rank, int *order)
{
    const PcmGraph G = graphs[blockIdx.y];
    if ((int)blockIdx.x * 256 >= G.C) return;
    __shared__ int sdeg[PCM_MAX_C];
    for (int k = (int)threadIdx.x; k < G.C; k += 256) sdeg[k] = deg[G.c0 + k];
    __syncthreads();
    const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (c >= G.C) return;
    const int mine = sdeg[c];
    int before = 0;
    for (int d = 0; d < G.C; ++d) { const int o = sdeg[d]; before += (o > mine || (o == mine && d < c)) ? 1 : 0; }
    rank[G.c0 + c] = before; order[G.c0 + before] = c;
}

/* a wave per row of the original matrix; grid (ceil(max C / 4), graphs) */
__global__ __launch_bounds__(256) void k_pcm_relabel(const PcmGraph *__restrict__ graphs, const unsigned long long *__restrict__ words, const int *__restrict__ rank,
                                                     const int *__restrict__ order, unsigned long long *rwords)
{
    const PcmGraph G = graphs[blockIdx.y];
    if ((int)blockIdx.x * 4 >= G.C) return;
    __shared__ int sorder[PCM_MAX_C];
    __shared__ unsigned long long srow[4][64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, c = (int)blockIdx.x * 4 + wave;
    for (int k = (int)threadIdx.x; k < G.C; k += 256) sorder[k] = order[G.c0 + k];
    srow[wave][lane] = (c < G.C && lane < G.W) ? words[G.woff + (size_t)c * G.W + lane] : 0ull;
    __syncthreads();
    if (c >= G.C || lane >= G.W) return;
    unsigned long long out = 0;
    for (int k = 0; k < 64; ++k) {
        const int b = (k + lane) & 63, n = lane * 64 + b;           /* new index n: bit b of this lane's word */
        if (n >= G.C) continue;
        const int o = sorder[n];
        out |= ((srow[wave][o >> 6] >> (o & 63)) & 1ull) << b;
    }
    rwords[G.woff + (size_t)rank[G.c0 + c] * G.W + lane] = out;
}

/* the greedy walk from start v over the matrix in rank order, by one wave: returns the size, M = the members' bits of this lane's word.
 * At most C steps: every step takes u out of U (the diagonal is zero, and the bit is cleared here as well) */
__device__ __forceinline__ int pcm_walk(const unsigned long long *__restrict__ rows, int W, int C, int v, int lane, unsigned long long &M)
{
    unsigned long long U = lane < W ? rows[(size_t)v * W + lane] : 0ull;
    M = (lane == (v >> 6)) ? 1ull << (v & 63) : 0ull;
    int size = 1;
    for (int step = 0; step < C; ++step) {
        const unsigned long long nz = __ballot(U != 0ull);
        if (nz == 0ull) break;
        const int L = __builtin_amdgcn_readfirstlane(__builtin_ctzll(nz));
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)U, L), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(U >> 32), L);
        const int b = lo ? __builtin_ctz(lo) : 32 + __builtin_ctz(hi), u = L * 64 + b;
        const unsigned long long N = lane < W ? rows[(size_t)u * W + lane] : 0ull;
        U &= N;
        if (lane == L) { M |= 1ull << b; U &= ~(1ull << b); }
        ++size;
    }
    return size;
}

/* a wave per start, starts in rank order; grid (ceil(max C / 4), graphs) */
__global__ __launch_bounds__(256) void k_pcm_clique(const PcmGraph *__restrict__ graphs, const unsigned long long *__restrict__ rwords, const int *__restrict__ deg,
                                                    const int *__restrict__ order, int *size, unsigned *best, unsigned long long *steps)
{
    const PcmGraph G = graphs[blockIdx.y];
    const int lane = (int)threadIdx.x & 63, v = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + ((int)threadIdx.x >> 6));
    if (v >= G.C) return;
    const int dv = deg[G.c0 + order[G.c0 + v]];
    const unsigned tie = (unsigned)(PCM_MAX_C - 1 - v);
    const unsigned reach = ((unsigned)(dv + 1) << PCM_KEY_BITS) | tie;          /* the best key this start could publish */
    const unsigned seen = __hip_atomic_load(best + blockIdx.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (reach < seen) { if (lane == 0) size[G.c0 + v] = 0; return; }            /* it can neither win nor tie ahead of that start */
    unsigned long long M;
    const int n = pcm_walk(rwords + G.woff, G.W, G.C, v, lane, M);
    if (lane == 0) {
        size[G.c0 + v] = n;
        atomicMax(best + blockIdx.y, ((unsigned)n << PCM_KEY_BITS) | tie);
        atomicAdd(steps + blockIdx.y, (unsigned long long)(n - 1));
    }
}

/* a workgroup per graph */
__global__ __launch_bounds__(256) void k_pcm_pick(const PcmGraph *__restrict__ graphs, const unsigned long long *__restrict__ rwords, const int *__restrict__ deg,
                                                  const int *__restrict__ order, const int *__restrict__ size, unsigned char *sel, ll_pcm_record *rec)
{
    const PcmGraph G = graphs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    __shared__ unsigned skey[256];
    __shared__ long long sdeg[256];
    __shared__ int smax[256];
    unsigned key = 0; long long dsum = 0; int dmax = 0;
    for (int k = tid; k < G.C; k += 256) {
        sel[G.c0 + k] = 0;
        key = max(key, ((unsigned)size[G.c0 + k] << PCM_KEY_BITS) | (unsigned)(PCM_MAX_C - 1 - k));
        const int d = deg[G.c0 + k];
        dsum += d; dmax = max(dmax, d);
    }
    skey[tid] = key; sdeg[tid] = dsum; smax[tid] = dmax;
    for (int o = 128; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) { skey[tid] = max(skey[tid], skey[tid + o]); sdeg[tid] += sdeg[tid + o]; smax[tid] = max(smax[tid], smax[tid + o]); }
    }
    __syncthreads();
    if (tid >= 64) return;
    ll_pcm_record R = {G.C, 0, -1, 0, 0};
    if (G.C > 0) {
        const int v = PCM_MAX_C - 1 - (int)(skey[0] & (unsigned)(PCM_MAX_C - 1));
        unsigned long long M;
        R.n_selected = pcm_walk(rwords + G.woff, G.W, G.C, v, tid, M);
        R.start = order[G.c0 + v]; R.max_degree = smax[0]; R.n_consistent_pairs = sdeg[0] / 2;
        while (M) { const int b = __builtin_ctzll(M); M &= M - 1; sel[G.c0 + order[G.c0 + tid * 64 + b]] = 1; }
    }
    if (tid == 0) rec[blockIdx.x] = R;
}

/* ------------------------------------------------------------------ host side */
static int pcm_fail(ll_pcm *v, int rc, const std::string &msg) { v->err = "pcm: " + msg; return rc; }
#define PCM_HIP(call) LL_HIP_CHECK(pcm_fail, v, "", call, #call)

extern "C" void ll_pcm_default_params(ll_pcm_params *p)
{
    if (!p) return;
    p->rot_tol = 0.05; p->trans_tol = 0.5; p->rot_rate = 2e-4; p->trans_rate = 0.02;
}

static size_t pcm_up_bytes(size_t G, size_t N, size_t Ct)
{
    return ll_up256(N * 7 * sizeof(double)) + ll_up256(N * sizeof(double)) + ll_up256(Ct * sizeof(PcmCand)) + ll_up256(G * sizeof(PcmGraph));
}

static size_t pcm_carve(ll_pcm *v, unsigned char *base)
{
    LLCarve C{base};
    const size_t G = (size_t)v->max_graphs, Ct = (size_t)v->max_cands;
    v->d_up = C.take<unsigned char>(v->up_bytes);
    v->d_prep = C.take<double>(Ct * PCM_PREP);
    v->d_deg = C.take<int>(Ct); v->d_rank = C.take<int>(Ct); v->d_order = C.take<int>(Ct); v->d_size = C.take<int>(Ct);
    v->d_sel = C.take<unsigned char>(Ct);
    v->d_rec = C.take<ll_pcm_record>(G);
    v->d_steps = C.take<unsigned long long>(G + (G + 1) / 2);      /* the steps, then the best keys (4 bytes each) */
    v->d_best = base ? (unsigned *)(v->d_steps + G) : nullptr;
    return C.at;
}

extern "C" void ll_pcm_destroy(ll_pcm *v)
{
    if (!v) return;
    if (v->ctx) { (void)hipSetDevice(v->ctx->device); (void)hipStreamSynchronize(v->ctx->stream); }
    if (v->d_mem) (void)hipFree(v->d_mem);
    if (v->d_words) (void)hipFree(v->d_words);
    for (hipEvent_t e : v->ev) if (e) (void)hipEventDestroy(e);
    delete v;
}

extern "C" int ll_pcm_create(ll_ctx *ctx, int max_graphs, int max_nodes_total, int max_candidates_total, ll_pcm **out)
{
    if (!ctx || !out) return LL_ERR_ARG;
    *out = nullptr;
    if (max_graphs < 1 || max_graphs > 65535 || max_nodes_total < 1 || max_nodes_total > (1 << 26) || max_candidates_total < 0 || max_candidates_total > (1 << 24)) {
        ctx->err = "pcm: max_graphs outside 1 .. 65535, max_nodes_total outside 1 .. 2^26 or max_candidates_total outside 0 .. 2^24";
        return LL_ERR_ARG;
    }
    LL_HIP(hipSetDevice(ctx->device));
    ll_pcm *v = new ll_pcm();
    v->ctx = ctx; v->max_graphs = max_graphs; v->max_nodes = max_nodes_total; v->max_cands = max_candidates_total;
    v->up_bytes = pcm_up_bytes((size_t)max_graphs, (size_t)max_nodes_total, (size_t)max_candidates_total);
    const size_t bytes = pcm_carve(v, nullptr);
    bool ok = hipMalloc((void **)&v->d_mem, bytes) == hipSuccess;
    for (hipEvent_t &e : v->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ll_pcm_destroy(v);
        ctx->err = "pcm: allocation failed (" + std::to_string(bytes) + " bytes)";
        return LL_ERR_HIP;
    }
    pcm_carve(v, v->d_mem);
    *out = v;
    return LL_OK;
}

extern "C" const char *ll_pcm_last_error(const ll_pcm *v) { return v ? v->err.c_str() : "pcm: NULL handle"; }

/* the checks run and select share: counts, offsets, the limits; fills the graphs' table */
static int pcm_layout(ll_pcm *v, int n_graphs, const int *cand_off, std::vector<PcmGraph> &tab)
{
    if (n_graphs < 0 || !cand_off) return pcm_fail(v, LL_ERR_ARG, "n_graphs < 0, or an offset array is NULL");
    if (n_graphs > v->max_graphs) return pcm_fail(v, LL_ERR_CAPACITY, std::to_string(n_graphs) + " graphs exceed max_graphs " + std::to_string(v->max_graphs));
    if (cand_off[0] != 0) return pcm_fail(v, LL_ERR_ARG, "offsets must start at 0");
    for (int g = 0; g < n_graphs; ++g)
        if (cand_off[g + 1] < cand_off[g]) return pcm_fail(v, LL_ERR_ARG, "graph " + std::to_string(g) + ": offsets do not ascend");
    if (cand_off[n_graphs] > v->max_cands)
        return pcm_fail(v, LL_ERR_CAPACITY, std::to_string(cand_off[n_graphs]) + " candidates exceed max_candidates_total " + std::to_string(v->max_cands));
    tab.resize((size_t)n_graphs);
    long long woff = 0;
    for (int g = 0; g < n_graphs; ++g) {
        const int C = cand_off[g + 1] - cand_off[g];
        if (C > PCM_MAX_C) return pcm_fail(v, LL_ERR_CAPACITY, "graph " + std::to_string(g) + ": " + std::to_string(C) + " candidates, a graph takes at most " + std::to_string(PCM_MAX_C));
        const PcmGraph G = {woff, cand_off[g], C, (C + 63) / 64, 0};
        tab[g] = G;
        woff += (long long)C * G.W;
    }
    return LL_OK;
}

static bool pcm_params_ok(const ll_pcm_params &p)
{
    const double t[4] = {p.rot_tol, p.trans_tol, p.rot_rate, p.trans_rate};
    for (int k = 0; k < 4; ++k) if (!std::isfinite(t[k]) || t[k] < 0.0) return false;
    return true;
}

/* one graph's poses and candidates checked; msg: what is wrong ("" if nothing) */
static std::string pcm_check_graph(int n, const double *poses, int C, const ll_pcm_candidate *cand)
{
    for (int k = 0; k < n; ++k) {
        if (!ll_finite_n(poses + (size_t)k * 7, 7)) return "node " + std::to_string(k) + ": the pose is not finite";
        if (ll_zero_quat(poses + (size_t)k * 7)) return "node " + std::to_string(k) + ": zero quaternion";
    }
    for (int c = 0; c < C; ++c) {
        const ll_pcm_candidate &e = cand[c];
        const std::string cs = "candidate " + std::to_string(c);
        if (e.i < 0 || e.i >= n || e.j < 0 || e.j >= n) return cs + ": a node index lies outside the graph";
        if (e.i == e.j) return cs + ": i == j";
        if (!ll_finite_n(e.Z_w7, 7)) return cs + ": the measurement is not finite";
        if (ll_zero_quat(e.Z_w7)) return cs + ": zero quaternion";
    }
    return "";
}

/* normalised poses and the path length s of one graph */
static void pcm_host_nodes(int n, const double *poses, double *P, double *s)
{
    for (int k = 0; k < n; ++k) ll_pose_unit(poses + (size_t)k * 7, P + (size_t)k * 7);
    for (int k = 0; k < n; ++k) {
        if (k == 0) { s[0] = 0.0; continue; }
        const double dx = P[k * 7 + 4] - P[(k - 1) * 7 + 4], dy = P[k * 7 + 5] - P[(k - 1) * 7 + 5], dz = P[k * 7 + 6] - P[(k - 1) * 7 + 6];
        s[k] = s[k - 1] + std::sqrt((dx * dx + dy * dy) + dz * dz);
    }
}

/* the uploads read the caller's (or this call's) pageable memory: a call that fails after enqueuing one waits for the stream before it returns */
struct PcmDrain {
    hipStream_t st; bool armed = true;
    ~PcmDrain() { if (armed) (void)hipStreamSynchronize(st); }
};

static int pcm_grow_words(ll_pcm *v, size_t words)
{
    if (words <= v->words_cap) return LL_OK;
    if (v->d_words) { (void)hipStreamSynchronize(v->ctx->stream); (void)hipFree(v->d_words); }
    v->d_words = nullptr; v->words_cap = 0; v->has_run = false;
    if (hipMalloc((void **)&v->d_words, words * 2 * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        v->d_words = nullptr;
        return pcm_fail(v, LL_ERR_HIP, "the bit-matrix workspace could not be allocated (" + std::to_string(words * 16) + " bytes)");
    }
    v->words_cap = words;
    return LL_OK;
}

/* stages 1 .. 4 on the matrices at d_words, the results, the one synchronisation.  ev[2] has been recorded by the caller */
static int pcm_select_and_read(ll_pcm *v, const std::vector<PcmGraph> &tab, const PcmGraph *d_graph, int maxC, unsigned char *selected, int *degree, ll_pcm_record *rec,
                               bool with_front)
{
    hipStream_t st = v->ctx->stream;
    const int G = (int)tab.size(), Ct = tab.empty() ? 0 : tab.back().c0 + tab.back().C;
    unsigned long long *rw = v->d_words + v->words_cap;
    const dim3 per4((unsigned)((maxC + 3) / 4), (unsigned)G), per256((unsigned)((maxC + 255) / 256), (unsigned)G);
    PCM_HIP(hipMemsetAsync(v->d_steps, 0, (size_t)v->max_graphs * (sizeof(unsigned long long) + sizeof(unsigned)), st));   /* the steps and, behind all of them, the best keys */
    hipLaunchKernelGGL(k_pcm_degree, per4, dim3(256), 0, st, d_graph, (const unsigned long long *)v->d_words, v->d_deg);
    hipLaunchKernelGGL(k_pcm_rank, per256, dim3(256), 0, st, d_graph, (const int *)v->d_deg, v->d_rank, v->d_order);
    hipLaunchKernelGGL(k_pcm_relabel, per4, dim3(256), 0, st, d_graph, (const unsigned long long *)v->d_words, (const int *)v->d_rank, (const int *)v->d_order, rw);
    PCM_HIP(hipEventRecord(v->ev[3], st));
    hipLaunchKernelGGL(k_pcm_clique, per4, dim3(256), 0, st, d_graph, (const unsigned long long *)rw, (const int *)v->d_deg, (const int *)v->d_order, v->d_size, v->d_best, v->d_steps);
    PCM_HIP(hipEventRecord(v->ev[4], st));
    hipLaunchKernelGGL(k_pcm_pick, dim3((unsigned)G), dim3(256), 0, st, d_graph, (const unsigned long long *)rw, (const int *)v->d_deg, (const int *)v->d_order, (const int *)v->d_size,
                       v->d_sel, v->d_rec);
    PCM_HIP(hipEventRecord(v->ev[5], st));
    const size_t b_sel = ll_up256((size_t)Ct), b_deg = ll_up256((size_t)Ct * sizeof(int)), b_rec = ll_up256((size_t)G * sizeof(ll_pcm_record)), b_steps = (size_t)G * sizeof(unsigned long long);
    unsigned char *pin = (unsigned char *)ll_pinned_scratch(b_sel + b_deg + b_rec + b_steps);
    if (!pin) return pcm_fail(v, LL_ERR_HIP, "no page-locked scratch");
    PCM_HIP(hipMemcpyAsync(pin, v->d_sel, (size_t)Ct, hipMemcpyDeviceToHost, st));
    PCM_HIP(hipMemcpyAsync(pin + b_sel, v->d_deg, (size_t)Ct * sizeof(int), hipMemcpyDeviceToHost, st));
    PCM_HIP(hipMemcpyAsync(pin + b_sel + b_deg, v->d_rec, (size_t)G * sizeof(ll_pcm_record), hipMemcpyDeviceToHost, st));
    PCM_HIP(hipMemcpyAsync(pin + b_sel + b_deg + b_rec, v->d_steps, b_steps, hipMemcpyDeviceToHost, st));
    PCM_HIP(hipGetLastError());
    PCM_HIP(hipStreamSynchronize(st));
    std::memcpy(selected, pin, (size_t)Ct);
    if (degree) std::memcpy(degree, pin + b_sel, (size_t)Ct * sizeof(int));
    if (rec) std::memcpy(rec, pin + b_sel + b_deg, (size_t)G * sizeof(ll_pcm_record));
    const unsigned long long *steps = (const unsigned long long *)(pin + b_sel + b_deg + b_rec);
    v->ms[0] = with_front ? ll_event_ms(v->ev[0], v->ev[1], 0.0) : 0.0;
    v->ms[1] = with_front ? ll_event_ms(v->ev[1], v->ev[2], 0.0) : 0.0;
    for (int k = 2; k < 5; ++k) v->ms[k] = ll_event_ms(v->ev[k], v->ev[k + 1], 0.0);
    v->counts[0] = G; v->counts[1] = Ct; v->counts[2] = 0; v->counts[3] = 0;
    for (int g = 0; g < G; ++g) { if (with_front) v->counts[2] += (long long)tab[g].C * tab[g].C; v->counts[3] += (long long)steps[g]; }
    v->last = tab; v->has_run = true;
    return LL_OK;
}

/* a call without a candidate: nothing is launched */
static void pcm_empty(ll_pcm *v, const std::vector<PcmGraph> &tab, ll_pcm_record *rec)
{
    for (size_t g = 0; rec && g < tab.size(); ++g) { const ll_pcm_record R = {0, 0, -1, 0, 0}; rec[g] = R; }
    for (int k = 0; k < 5; ++k) v->ms[k] = 0.0;
    v->counts[0] = (long long)tab.size(); v->counts[1] = v->counts[2] = v->counts[3] = 0;
    v->last = tab; v->has_run = true;
}

extern "C" int ll_pcm_run(ll_pcm *v, int n_graphs, const int *node_off, const int *cand_off, const double *poses_w7, const ll_pcm_candidate *candidates,
                          const ll_pcm_params *params, unsigned char *selected, int *degree, ll_pcm_record *rec)
{
    if (!v) return LL_ERR_ARG;
    /* ---- every refusal before anything is enqueued or an output changes */
    if (!node_off) return pcm_fail(v, LL_ERR_ARG, "n_graphs < 0, or an offset array is NULL");
    std::vector<PcmGraph> tab;
    int rc = pcm_layout(v, n_graphs, cand_off, tab); if (rc) return rc;
    if (node_off[0] != 0) return pcm_fail(v, LL_ERR_ARG, "offsets must start at 0");
    for (int g = 0; g < n_graphs; ++g)
        if (node_off[g + 1] < node_off[g]) return pcm_fail(v, LL_ERR_ARG, "graph " + std::to_string(g) + ": offsets do not ascend");
    const int N = node_off[n_graphs], Ct = cand_off[n_graphs];
    if (N > v->max_nodes) return pcm_fail(v, LL_ERR_CAPACITY, std::to_string(N) + " nodes exceed max_nodes_total " + std::to_string(v->max_nodes));
    if ((N > 0 && !poses_w7) || (Ct > 0 && (!candidates || !selected))) return pcm_fail(v, LL_ERR_ARG, "poses, candidates or selected is NULL");
    ll_pcm_params P;
    if (params) P = *params; else ll_pcm_default_params(&P);
    if (!pcm_params_ok(P)) return pcm_fail(v, LL_ERR_ARG, "a parameter is negative or not finite");
    for (int g = 0; g < n_graphs; ++g) {
        const std::string msg = pcm_check_graph(node_off[g + 1] - node_off[g], poses_w7 + (size_t)node_off[g] * 7, tab[g].C, candidates + tab[g].c0);
        if (!msg.empty()) return pcm_fail(v, LL_ERR_ARG, "graph " + std::to_string(g) + ", " + msg);
    }
    if (Ct == 0) { pcm_empty(v, tab, rec); return LL_OK; }
    /* ---- the upload: normalised poses, path lengths, candidates with rows of the pose table, the graphs */
    const size_t o_pose = 0, o_s = o_pose + ll_up256((size_t)N * 7 * sizeof(double)), o_cand = o_s + ll_up256((size_t)N * sizeof(double)),
                 o_graph = o_cand + ll_up256((size_t)Ct * sizeof(PcmCand)), up = o_graph + ll_up256((size_t)n_graphs * sizeof(PcmGraph));
    std::vector<unsigned char> blob(up);
    double *hp = (double *)(blob.data() + o_pose), *hs = (double *)(blob.data() + o_s);
    PcmCand *hc = (PcmCand *)(blob.data() + o_cand);
    int maxC = 0;
    for (int g = 0; g < n_graphs; ++g) {
        const int n0 = node_off[g];
        pcm_host_nodes(node_off[g + 1] - n0, poses_w7 + (size_t)n0 * 7, hp + (size_t)n0 * 7, hs + n0);
        for (int c = tab[g].c0; c < tab[g].c0 + tab[g].C; ++c) {
            ll_pose_unit(candidates[c].Z_w7, hc[c].Z);
            hc[c].i = n0 + candidates[c].i; hc[c].j = n0 + candidates[c].j;
        }
        maxC = std::max(maxC, tab[g].C);
    }
    std::memcpy(blob.data() + o_graph, tab.data(), (size_t)n_graphs * sizeof(PcmGraph));
    hipStream_t st = v->ctx->stream;
    PCM_HIP(hipSetDevice(v->ctx->device));
    const size_t total = (size_t)(tab.back().woff + (long long)tab.back().C * tab.back().W);
    rc = pcm_grow_words(v, total); if (rc) return rc;
    PcmDrain drain{st};
    PCM_HIP(hipMemcpyAsync(v->d_up, blob.data(), up, hipMemcpyHostToDevice, st));
    const PcmGraph *d_graph = (const PcmGraph *)(v->d_up + o_graph);
    const PcmTol tol = {P.rot_tol, P.trans_tol, P.rot_rate, P.trans_rate};
    int max_tiles = 0;
    for (const PcmGraph &G : tab) max_tiles = std::max(max_tiles, (G.C + PCM_ROWS - 1) / PCM_ROWS * G.W);
    PCM_HIP(hipEventRecord(v->ev[0], st));
    hipLaunchKernelGGL(k_pcm_prepare, dim3((unsigned)((Ct + 255) / 256)), dim3(256), 0, st, (const double *)(v->d_up + o_pose), (const double *)(v->d_up + o_s),
                       (const PcmCand *)(v->d_up + o_cand), Ct, v->d_prep);
    PCM_HIP(hipEventRecord(v->ev[1], st));
    hipLaunchKernelGGL(k_pcm_adjacency, dim3((unsigned)max_tiles, (unsigned)n_graphs), dim3(PCM_ROWS), 0, st, d_graph, (const double *)v->d_prep, tol, v->d_words);
    PCM_HIP(hipEventRecord(v->ev[2], st));
    rc = pcm_select_and_read(v, tab, d_graph, maxC, selected, degree, rec, true);
    drain.armed = rc != LL_OK;
    return rc;
}

extern "C" int ll_pcm_select(ll_pcm *v, int n_graphs, const int *cand_off, const unsigned long long *words, unsigned char *selected, int *degree, ll_pcm_record *rec)
{
    if (!v) return LL_ERR_ARG;
    std::vector<PcmGraph> tab;
    int rc = pcm_layout(v, n_graphs, cand_off, tab); if (rc) return rc;
    const int Ct = cand_off[n_graphs];
    if (Ct > 0 && (!words || !selected)) return pcm_fail(v, LL_ERR_ARG, "words or selected is NULL");
    int maxC = 0;
    for (int g = 0; g < n_graphs; ++g) {
        const PcmGraph &G = tab[g];
        const unsigned long long *m = words + G.woff;
        const std::string gs = "graph " + std::to_string(g) + ", candidate ";
        for (int c = 0; c < G.C; ++c) {
            const unsigned long long *row = m + (size_t)c * G.W;
            if ((G.C & 63) && (row[G.W - 1] >> (G.C & 63))) return pcm_fail(v, LL_ERR_ARG, gs + std::to_string(c) + ": a bit at or beyond the number of candidates");
            if ((row[c >> 6] >> (c & 63)) & 1ull) return pcm_fail(v, LL_ERR_ARG, gs + std::to_string(c) + ": a bit on the diagonal");
            for (int w = 0; w < G.W; ++w)
                for (unsigned long long b = row[w]; b; b &= b - 1) {
                    const int d = w * 64 + __builtin_ctzll(b);
                    if (!((m[(size_t)d * G.W + (c >> 6)] >> (c & 63)) & 1ull)) return pcm_fail(v, LL_ERR_ARG, gs + std::to_string(c) + ": the matrix is not symmetric at column " + std::to_string(d));
                }
        }
        maxC = std::max(maxC, G.C);
    }
    if (Ct == 0) { pcm_empty(v, tab, rec); return LL_OK; }
    hipStream_t st = v->ctx->stream;
    PCM_HIP(hipSetDevice(v->ctx->device));
    const size_t total = (size_t)(tab.back().woff + (long long)tab.back().C * tab.back().W);
    rc = pcm_grow_words(v, total); if (rc) return rc;
    PcmDrain drain{st};
    PCM_HIP(hipMemcpyAsync(v->d_up, tab.data(), (size_t)n_graphs * sizeof(PcmGraph), hipMemcpyHostToDevice, st));
    PCM_HIP(hipMemcpyAsync(v->d_words, words, total * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    PCM_HIP(hipEventRecord(v->ev[2], st));
    rc = pcm_select_and_read(v, tab, (const PcmGraph *)v->d_up, maxC, selected, degree, rec, false);
    drain.armed = rc != LL_OK;
    return rc;
}

extern "C" int ll_pcm_adjacency(ll_pcm *v, int graph, unsigned long long *words_out)
{
    if (!v) return LL_ERR_ARG;
    if (!v->has_run) return pcm_fail(v, LL_ERR_STATE, "adjacency: there is no run or select to read");
    if (graph < 0 || graph >= (int)v->last.size()) return pcm_fail(v, LL_ERR_ARG, "adjacency: the last call had " + std::to_string(v->last.size()) + " graphs, there is no graph " + std::to_string(graph));
    const PcmGraph &G = v->last[graph];
    if (G.C == 0) return LL_OK;
    if (!words_out) return pcm_fail(v, LL_ERR_ARG, "adjacency: words_out is NULL");
    PCM_HIP(hipSetDevice(v->ctx->device));
    PCM_HIP(hipMemcpyAsync(words_out, v->d_words + G.woff, (size_t)G.C * G.W * sizeof(unsigned long long), hipMemcpyDeviceToHost, v->ctx->stream));
    PCM_HIP(hipStreamSynchronize(v->ctx->stream));
    return LL_OK;
}

extern "C" int ll_pcm_timing(const ll_pcm *v, double *ms, long long *counts)
{
    if (!v) return LL_ERR_ARG;
    if (ms) for (int k = 0; k < 5; ++k) ms[k] = v->ms[k];
    if (counts) for (int k = 0; k < 4; ++k) counts[k] = v->counts[k];
    return LL_OK;
}

/* ------------------------------------------------------------------ one graph on the host: the same pair arithmetic, the selection as the header states it */
extern "C" int ll_pcm_host(int n_nodes, const double *poses_w7, int C, const ll_pcm_candidate *candidates, const ll_pcm_params *params,
                           unsigned long long *words_out, unsigned char *selected, int *degree, ll_pcm_record *rec)
{
    if (n_nodes < 0 || C < 0 || (n_nodes > 0 && !poses_w7) || (C > 0 && (!candidates || !selected))) return LL_ERR_ARG;
    if (C > PCM_MAX_C) return LL_ERR_CAPACITY;
    ll_pcm_params P;
    if (params) P = *params; else ll_pcm_default_params(&P);
    if (!pcm_params_ok(P)) return LL_ERR_ARG;
    if (!pcm_check_graph(n_nodes, poses_w7, C, candidates).empty()) return LL_ERR_ARG;
    const ll_pcm_record empty = {0, 0, -1, 0, 0};
    if (C == 0) { if (rec) *rec = empty; return LL_OK; }
    const int W = (C + 63) / 64;
    std::vector<double> Pn((size_t)n_nodes * 7), s((size_t)n_nodes), prep((size_t)C * PCM_PREP);
    pcm_host_nodes(n_nodes, poses_w7, Pn.data(), s.data());
    for (int c = 0; c < C; ++c) {
        double Z[7];
        ll_pose_unit(candidates[c].Z_w7, Z);
        pcm_prepare(&Pn[(size_t)candidates[c].i * 7], &Pn[(size_t)candidates[c].j * 7], Z, s[candidates[c].i], s[candidates[c].j], &prep[(size_t)c * PCM_PREP]);
    }
    const PcmTol tol = {P.rot_tol, P.trans_tol, P.rot_rate, P.trans_rate};
    std::vector<unsigned long long> m((size_t)C * W, 0ull), rm((size_t)C * W, 0ull);
    std::vector<int> deg((size_t)C, 0), order((size_t)C), rank((size_t)C);
    for (int c = 0; c < C; ++c)
        for (int d = c + 1; d < C; ++d) {
            const double *a = &prep[(size_t)c * PCM_PREP], *b = &prep[(size_t)d * PCM_PREP];
            if (!pcm_pair(a, a + 14, a[21], a[22], b + 7, b[21], b[22], tol)) continue;
            m[(size_t)c * W + (d >> 6)] |= 1ull << (d & 63); m[(size_t)d * W + (c >> 6)] |= 1ull << (c & 63);
            ++deg[c]; ++deg[d];
        }
    for (int c = 0; c < C; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return deg[a] > deg[b]; });
    for (int r = 0; r < C; ++r) rank[order[r]] = r;
    for (int c = 0; c < C; ++c)
        for (int w = 0; w < W; ++w)
            for (unsigned long long b = m[(size_t)c * W + w]; b; b &= b - 1) {
                const int rd = rank[w * 64 + __builtin_ctzll(b)];
                rm[(size_t)rank[c] * W + (rd >> 6)] |= 1ull << (rd & 63);
            }
    /* every start in the order; a later start must be strictly larger to win, so one whose degree + 1 is not is skipped */
    std::vector<unsigned long long> U((size_t)W), M((size_t)W), bestM((size_t)W, 0ull);
    int best = 0, best_v = -1;
    long long pairs = 0;
    for (int c = 0; c < C; ++c) pairs += deg[c];
    for (int v = 0; v < C; ++v) {
        if (deg[order[v]] + 1 <= best) continue;
        for (int w = 0; w < W; ++w) { U[w] = rm[(size_t)v * W + w]; M[w] = 0ull; }
        M[v >> 6] |= 1ull << (v & 63);
        int size = 1;
        for (;;) {
            int w = 0;
            while (w < W && U[w] == 0ull) ++w;
            if (w == W) break;
            const int u = w * 64 + __builtin_ctzll(U[w]);
            M[u >> 6] |= 1ull << (u & 63);
            for (int k = 0; k < W; ++k) U[k] &= rm[(size_t)u * W + k];
            U[u >> 6] &= ~(1ull << (u & 63));
            ++size;
        }
        if (size > best) { best = size; best_v = v; bestM = M; }
    }
    for (int c = 0; c < C; ++c) selected[c] = (unsigned char)((bestM[rank[c] >> 6] >> (rank[c] & 63)) & 1ull);
    if (degree) for (int c = 0; c < C; ++c) degree[c] = deg[c];
    if (words_out) std::memcpy(words_out, m.data(), m.size() * sizeof(unsigned long long));
    if (rec) { const ll_pcm_record R = {C, best, order[best_v], deg[order[0]], pairs / 2}; *rec = R; }
    return LL_OK;
}
