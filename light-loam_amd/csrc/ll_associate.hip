/*
 * ll_associate.hip -- a5 + a6 + a7: TransformToStart, K=1 nearest neighbour, ring-window second / third point.
 * Replaces laserOdometry.cpp:77-95, :491-620 (corners), :653-793 (planes) and the kd-tree rebuild :895-896
 * of /root/reference.
 *
 * Targets of slot s are the less-sharp / less-flat clouds of slot s-1, still resident in HBM from the
 * extract stage (no publish -> subscribe -> fromROSMsg -> kd-tree build).
 *
 * k_build_grid (one workgroup per (scan, cloud)) builds what replaces the kd-tree:
 *   - a uniform 2-D (x, y) cell grid: LDS histogram over 128 x 128 cells of 1 m, exclusive scan, scatter of
 *     (x, y, z, place << 8 | ring) into cell order -- a point's PLACE is its float4 offset in the slot's cloud: its index for a
 *     contiguous cloud, ring * ring_cap + k for the ring rows of an extracted less-flat cloud (ll_common.h); places order like
 *     the reference's indices.  Points outside +-64 m saturate into the border cells, whose rectangles are treated as
 *     unbounded outwards;
 *   - for an extracted slot, first: the rings' counts -> the prefix table lf_pre (place -> index) and the header's four totals;
 *   - ring tables first_ge[v] = min{j : ring_j >= v}, last_le[v] = max{j : ring_j <= v} (ring_j = int(intensity_j))
 *     and a flag saying whether they reproduce the reference's sequential walk bounds for EVERY start index
 *     (true whenever ring ids never run more than NEARBY_SCAN ahead/behind of their position, as in any cloud
 *     the extract stage produces; arbitrary user targets may clear it).
 * k_associate, 8 lanes per query (one 128-byte line of cell-ordered points per step):
 *   K=1 search   cells visited in Chebyshev rings around the query's cell, a cell skipped only when its rectangle
 *                is provably farther than the best so far, the ring loop stopped when the whole next ring is.
 *                Distance = FLANN L2_Simple in f32 ((dx*dx + dy*dy) + dz*dz, no FMA); equal distances -> lowest
 *                place = lowest original index (traversal-dependent in the kd-tree; defined here and in the oracle).  Only
 *                neighbours closer than DISTANCE_SQ_THRESHOLD are ever used (:497 / :659): at most 7 rings.
 *   ring walks   (:504-553, :668-721) are sequential loops over a contiguous index window with early breaks and a
 *                running minimum under strict '<'.  With valid tables the window is (last_le[..], first_ge[..]),
 *                and the result is the lexicographic minimum of (distance, visiting order) over the window points
 *                of the right ring class -- found with the same pruned cell search instead of scanning ~2500
 *                points per query.  Without valid tables the wave-cooperative sequential scan below is used
 *                (break = ballot of "first lane whose ring leaves the +-2.5 window").  Both are exact.
 */
#include "ll_associate.h"

extern __shared__ __attribute__((aligned(16))) unsigned char ll_gsm[];

#ifdef LL_PHASE_TIMING   /* tools/phase_timing.py: V.dbg[8..11] = k_build_grid phases, V.dbg[14] = its workgroups */
#define LL_GPHASE_BEGIN() long long ll_t0 = (tid == 0) ? (long long)__builtin_amdgcn_s_memtime() : 0
#define LL_GPHASE(i) do { __syncthreads(); if (tid == 0) { const long long t1 = (long long)__builtin_amdgcn_s_memtime(); \
    atomicAdd(&V.dbg[i], (unsigned long long)(t1 - ll_t0)); ll_t0 = t1; if ((i) == 11) atomicAdd(&V.dbg[14], 1ull); } } while (0)
#else
#define LL_GPHASE_BEGIN() do {} while (0)
#define LL_GPHASE(i) do {} while (0)
#endif

/* grid + ring tables of a target cloud; carry != 0: the carry clouds, else slot first + blockIdx/2.
 *
 * The cloud is read as CHUNKS of 64 consecutive points, one chunk per wave and load: a contiguous cloud (less-sharp; the carry; an
 * uploaded less-flat cloud) is chunk c = points [64 c, 64 c + 64); the ring-strided less-flat cloud of an extracted slot
 * (ll_common.h) is, ring after ring, the ceil(ring_nlf[r] / 64) chunks of ring r's row; the chunks are dealt to the sixteen waves in
 * equal blocks, so all of them stay busy whatever the rings' lengths.  A point is named by its PLACE (float4 offset inside the slot's
 * array; = index for a contiguous cloud): place order = index order, and every consumer of the grid only compares.
 * For an extracted slot this kernel is also where the scan's totals become known: the workgroup of the less-flat cloud scans the
 * per-ring counts into lf_pre and writes the four totals of the header (no ring of k_ring_features waited for another to learn them). */
#define LL_GB 1024      /* threads: one workgroup per CU (below), which is why the LDS beside the 68 KB histogram is free for the waves' stashes */
/* Workgroups per CU.  Two 1024-thread workgroups are 8 waves per SIMD, and the hardware admits the eighth wave only below 81 SGPRs
 * (MI355X_MICROARCH.md, residency: floor(800 / (ceil(sgpr / 16) * 16 + 16)) waves per SIMD; the occupancy query says 8 up to 96):
 * rounds 1-4 compiled this kernel to 82 SGPRs, so ONE workgroup per CU was resident whatever the occupancy report said.  Round 5
 * measured both on one box (profiles/r05_experiments/ab_build_grid_*.log): bound to 8 waves (78 SGPRs, two resident workgroups, 4 loads
 * in flight per lane) 9.4-9.7 ms per 16384 scans, left at one workgroup with 8 loads in flight 8.9-9.2 -- every phase of the kernel
 * takes 1.8-2.7x as long with a neighbour on the CU (instrumented build): it is bound by what a CU's LDS and memory pipes deliver,
 * not by latency a second workgroup could hide. */
#ifndef LL_GRID_WAVES
#define LL_GRID_WAVES 4
#endif
#ifndef LL_GRID_UN
#define LL_GRID_UN 8          /* chunks per batch = independent loads in flight per lane */
#endif
#ifndef LL_GRID_KEEP
#define LL_GRID_KEEP 3        /* batches a wave keeps in registers between the two sweeps */
#endif
#define LL_GRID_HIST_BYTES ((LL_GRID_NC + LL_GRID_NC / 16) * sizeof(int))
/* dynamic LDS: the histogram, then the waves' stashes -- `stash` chunks of 64 whole points (1 KB) for each of the LL_GB / 64 waves */
static size_t ll_grid_lds_bytes(int stash) { return LL_GRID_HIST_BYTES + (size_t)(LL_GB / 64) * stash * 64 * sizeof(float4); }
__global__ __launch_bounds__(LL_GB, LL_GRID_WAVES) void k_build_grid(LLView V, int first, int count, int carry, int stash)
{
    const int which = blockIdx.x & 1, sl = blockIdx.x >> 1;
    if (sl >= count) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NW = LL_GB / 64;
    /* cell c lives at hist[c + (c >> 4)]: the per-thread scan below walks 16 consecutive cells per lane, and the
     * one-word skew per 16 cells spreads the lanes over all LDS banks instead of putting them on two */
#define LL_HI(c) ((c) + ((c) >> 4))
    int *hist = (int *)ll_gsm;                      /* [LL_GRID_NC + LL_GRID_NC / 16] */
    __shared__ int sc[LL_GB / 64];
    __shared__ int feq[LL_TAB + 1], leq[LL_TAB + 1];
    __shared__ int okflag;
    __shared__ int rcnt[LL_MAX_RINGS], pre[LL_MAX_RINGS + 1], cpre[LL_MAX_RINGS + 1];   /* per ring: points, index of the first, chunk of the first */
    __shared__ int tot3[3];
    for (int i = tid; i < LL_GRID_NC + LL_GRID_NC / 16; i += LL_GB) hist[i] = 0;
    for (int i = tid; i <= LL_TAB; i += LL_GB) { feq[i] = INT_MAX; leq[i] = -1; }
    if (tid == 0) okflag = (V.nearby >= 0.0) ? 1 : 0;
    if (tid < 3) tot3[tid] = 0;

    const float4 *pts; int m = 0; int *gstart; float4 *gpts;
    bool extracted = false;                                /* an extracted slot: the counts are per ring, the totals not yet known */
    int s = 0;
    /* the per-ring counts are requested together with the header, before it is known whether they will be wanted (an extracted slot):
     * one round trip at the head of the workgroup instead of two */
    unsigned pc_spec = 0u; int nlf_spec = 0;
    if (!carry && tid < V.R) { const size_t o = (size_t)(first + sl) * V.R + tid; pc_spec = V.ring_cnt[o]; nlf_spec = V.ring_nlf[o]; }
    if (carry) {
        pts = which ? V.carry_surf : V.carry_corner; m = V.carry_cnt[which];
        gstart = V.carry_gstart + (size_t)which * LL_GSTRIDE;
        gpts = which ? V.carry_gpts_s : V.carry_gpts_c;
    } else {
        s = first + sl;
        const ScanHdr h = V.hdr[s];
        pts = which ? V.lflat + (size_t)s * V.LFS : V.lsharp + (size_t)s * V.cap_lsharp;
        gstart = V.gstart + ((size_t)s * 2 + which) * LL_GSTRIDE;
        gpts = which ? V.gpts_s + (size_t)s * V.NP : V.gpts_c + (size_t)s * V.cap_lsharp;
        if (h.status != 0) m = 0;
        else if (!h.lf_strided) m = which ? h.n_less_flat : h.n_less_sharp;         /* ll_upload_features: the caller's counts */
        else extracted = true;
    }
    __syncthreads();
    LL_GPHASE_BEGIN();
    if (extracted) {
        /* the rings' counts: less-flat points (k_ring_features) or less-sharp picks (k_ring_pick) of every ring; the workgroup of
         * the less-flat cloud also sums the three small clouds' counts for the header */
        const int R = V.R;
        if (tid < LL_MAX_RINGS) {
            const unsigned pc = pc_spec;
            rcnt[tid] = which ? nlf_spec : (int)((pc >> 8) & 0xffu);
            if (which) {
                const int a = ll_wave_sum_i32((int)(pc & 0xffu)), b = ll_wave_sum_i32((int)((pc >> 8) & 0xffu)), c = ll_wave_sum_i32((int)((pc >> 16) & 0xffu));
                if (lane == 0) { atomicAdd(&tot3[0], a); atomicAdd(&tot3[1], b); atomicAdd(&tot3[2], c); }
            }
        }
        __syncthreads();
        if (tid < 64) {                                    /* wave 0: exclusive prefixes of the points and of the 64-point chunks, two halves */
            int carry_p = 0, carry_c = 0;
            for (int half = 0; half * 64 < R; ++half) {                /* rings beyond R hold nothing: their prefixes are the totals (below) */
                const int q = half * 64 + lane;
                const int v = rcnt[q], c = (v + 63) >> 6;
                const int ip = ll_wave_incl_scan(v), ic = ll_wave_incl_scan(c);
                pre[q] = carry_p + ip - v; cpre[q] = carry_c + ic - c;
                carry_p += __builtin_amdgcn_readlane(ip, 63); carry_c += __builtin_amdgcn_readlane(ic, 63);
            }
            for (int q = (R + 63) / 64 * 64 + lane; q <= LL_MAX_RINGS; q += 64) { pre[q] = carry_p; cpre[q] = carry_c; }   /* incl. [LL_MAX_RINGS]: the totals */
        }
        __syncthreads();
        m = pre[LL_MAX_RINGS];
        if (which) {
            /* rings beyond R hold no point: pre[R] = the total.  lf_pre: what turns a place into the reference's index (C ABI, carry copy) */
            if (tid <= R) V.lf_pre[(size_t)s * (R + 1) + tid] = pre[tid];
            if (tid == 0) { ScanHdr *hh = &V.hdr[s]; hh->n_sharp = tot3[0]; hh->n_less_sharp = tot3[1]; hh->n_flat = tot3[2]; hh->n_less_flat = m; }
        }
        __syncthreads();
    }
    const bool strided = extracted && which != 0;
    const int stride = V.ring_cap;
    const int pend = strided ? V.R * stride : m;           /* one past the last place */
    const int nch = strided ? cpre[LL_MAX_RINGS] : (m + 63) >> 6;
    /* Every wave takes a BLOCK of consecutive chunks and walks it with a cursor (ring q, chunk k of that ring, the ring's length): the
     * next chunk is k + 1 or the first chunk of the next ring that holds a point -- scalar arithmetic, one LDS read per ring crossed,
     * nothing per chunk (a per-chunk lookup table cost the sweeps 15 % of their time). */
    const int per_wave = (nch + NW - 1) / NW;
    const int cw0 = min(nch, wave * per_wave), cw1 = min(nch, cw0 + per_wave);
    struct Cursor { int q, k, len, next_len; };     /* next_len: the following ring's length, read ahead (a VGPR holding a uniform value:
                                                      * the LDS read is waited for at the next crossing, not where it is issued) */
    auto ring_len = [&](int q) -> int { return q < LL_MAX_RINGS ? rcnt[q] : 1; };    /* beyond the table: a stopper for the skip loop */
    auto cursor_at = [&](int c) __attribute__((always_inline)) -> Cursor {       /* chunk c of the cloud (c < nch) */
        Cursor cu; cu.q = 0; cu.k = c; cu.len = m; cu.next_len = 0;
        if (strided) {
            int lo = 0, hi = V.R;                                                 /* the last ring whose first chunk is <= c (it holds a chunk: cpre[q + 1] > c) */
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (__builtin_amdgcn_readfirstlane(cpre[mid]) <= c) lo = mid; else hi = mid; }
            cu.q = lo; cu.k = c - __builtin_amdgcn_readfirstlane(cpre[lo]); cu.len = __builtin_amdgcn_readfirstlane(rcnt[lo]);
            cu.next_len = ring_len(lo + 1);
        }
        return cu;
    };
    /* the cursor's chunk -> its first place and the points it holds; then on to the next chunk */
    auto take = [&](Cursor &cu, int &place0, int &nv) __attribute__((always_inline)) {
        if (strided) {
            place0 = cu.q * stride + cu.k * 64; nv = cu.len - cu.k * 64;
            if (++cu.k * 64 >= cu.len) {
                cu.k = 0;
                do { ++cu.q; cu.len = __builtin_amdgcn_readfirstlane(cu.next_len); cu.next_len = ring_len(cu.q + 1); } while (cu.len == 0);
            }
        } else { place0 = cu.k * 64; nv = m - cu.k * 64; ++cu.k; }
    };
    constexpr int UN = LL_GRID_UN;                   /* independent loads in flight per lane */
/* One UNCONDITIONAL wait behind a batch of predicated loads.  Left to itself the compiler waits inside each `if (lane < nv)` block that
 * uses a point; on the path around the block nothing was waited for, so at the join the destination registers still count as "in
 * flight", and the next batch's address arithmetic -- which reuses them -- gets an s_waitcnt vmcnt(0) in front of EVERY load: one load
 * in flight instead of UN (the sweeps ran 2.2x slower than the flat loops they replaced until this line went in). */
#define LL_LOADS_LANDED() __builtin_amdgcn_s_waitcnt(0x0f70)                              /* vmcnt(0) */
#define LL_WSHR1(x) __builtin_amdgcn_update_dpp(0, (int)(x), 0x138, 0xf, 0xf, false)      /* wave_shr:1: lane i <- lane i - 1 */
#define LL_WSHL1(x) __builtin_amdgcn_update_dpp(0, (int)(x), 0x130, 0xf, 0xf, false)      /* wave_shl:1: lane i <- lane i + 1 */
    bool bad = false;
    /* histogram + ring tables from a chunk's keys (cell | ring value << 16) */
    auto count_chunk = [&](unsigned kv, int place0, int nv) __attribute__((always_inline)) {
        const bool in = lane < nv;
        if (in) atomicAdd(&hist[LL_HI((int)(kv & 0xFFFFu))], 1);
        /* ring tables, same sweep: first / last place of every ring value (only run boundaries touch LDS) */
        const int r = in ? (int)(kv >> 16) : 0;
        const bool oob = in && r >= LL_TAB;                                   /* 0xFF: int(intensity) outside [0, LL_TAB) */
        if (oob) bad = true;
        const int rprev = LL_WSHR1(r), rnext = LL_WSHL1(r);
        if (in && !oob) {
            const int place = place0 + lane;
            if (lane == 0 || r != rprev) atomicMin(&feq[r], place);
            if (lane == 63 || lane == nv - 1 || r != rnext) atomicMax(&leq[r], place);
        }
    };
    /* Both sweeps walk the wave's chunks in BATCHES of UN (load UN chunks, wait, process them), and what the histogram sweep has read
     * of the END of the wave's block the scatter sweep does not read again -- the kernel is held by its traffic:
     *   - the last LL_GRID_KEEP batches stay in registers, narrowed to what the scatter sweep wants of a point: x, y, z and the low byte
     *     of int(w) (four chunks' bytes to a register), their places and counts packed into one scalar per chunk.  The histogram
     *     sweep takes its ring key from the full w first (ll_grid_key): the tables and the out-of-range flag never see the byte;
     *   - the `stash` chunks in front of them wait in the wave's private piece of the LDS the workgroup leaves free (whole points);
     *   - only what lies in front of the stash is fetched again.
     * A cloud of at most LL_GRID_KEEP UN + stash chunks per wave is read once (every less-sharp cloud; with 5 stashed chunks the
     * headline's less-flat cloud, 33 per wave, 1.12 times; round 7 kept two whole batches: 1.52).  The batches end-align with the
     * wave's block, so the one short batch is the FIRST and those that stay are full. */
    constexpr int KB = LL_GRID_KEEP, KC = KB * UN;
    static_assert(UN % 4 == 0 && KB >= 1 && KB <= 3, "four ring bytes to a register; one to three kept batches");
    const int nb = (cw1 - cw0 + UN - 1) / UN;            /* batches of this wave; batch j = chunks c0 + j UN ..., those >= cw0 */
    const int c0 = cw1 - nb * UN;
    const int ckeep = cw1 - min(nb, KB) * UN;            /* the kept batches start here (below cw0: the short batch is one of them) */
    const int cst = max(cw0, ckeep - stash);             /* the stash holds chunks [cst, ckeep); [cw0, cst) is read twice */
    float4 *const stw = (float4 *)(ll_gsm + LL_GRID_HIST_BYTES) + (size_t)wave * stash * 64;
    float4 p[UN]; int pl[UN], nv[UN];
    float kx[KC], ky[KC], kz[KC]; unsigned kr[KC / 4]; int kpn[KC];     /* kpn: place << 7 | points (<= 64); place < 2^24 */
    /* the cursor first, for all UN chunks, THEN the loads back to back: with the cursor's loop between two loads the compiler
     * waits for the first (s_waitcnt vmcnt(0) at the loop's head) before it issues the second -- one load in flight, not UN */
    auto load_batch = [&](Cursor &cu, int c) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < UN; ++u) { pl[u] = 0; nv[u] = 0; if (c + u >= cw0) take(cu, pl[u], nv[u]); }
#pragma unroll
        for (int u = 0; u < UN; ++u) if (lane < nv[u]) p[u] = pts[pl[u] + lane];
    };
    auto count_batch = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < UN; ++u) count_chunk(lane < nv[u] ? ll_grid_key(p[u]) : 0u, pl[u], nv[u]);
    };
    auto keep_batch = [&](auto J) __attribute__((always_inline)) {     /* the batch just counted -> kept batch J */
        constexpr int j = decltype(J)::value;
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            kx[j * UN + u] = p[u].x; ky[j * UN + u] = p[u].y; kz[j * UN + u] = p[u].z;
            kpn[j * UN + u] = (pl[u] << 7) | min(nv[u], 64);
        }
#pragma unroll
        for (int g = 0; g < UN / 4; ++g) {
            unsigned w = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) w |= (unsigned)((int)p[g * 4 + b].w & 0xFF) << (8 * b);
            kr[j * UN / 4 + g] = w;
        }
    };
    /* the head's speculative loads of the rings' counts are waited for only where an extracted slot uses them: on the other path
     * their registers would count as "in flight" all through the sweep, and wherever the allocator reuses one -- for a load's
     * address, say -- every load of a batch would wait for the one before it */
    LL_LOADS_LANDED();
    if (nb > 0) {
        Cursor cu = cursor_at(cw0);
        int c = c0;
        for (; c < ckeep; c += UN) {
            load_batch(cu, c); LL_LOADS_LANDED(); count_batch();
#pragma unroll
            for (int u = 0; u < UN; ++u) if (c + u >= cst) stw[(c + u - cst) * 64 + lane] = p[u];
        }
        if constexpr (KB >= 3) if (nb >= 3) { load_batch(cu, c); LL_LOADS_LANDED(); count_batch(); keep_batch(std::integral_constant<int, KB - 3>{}); c += UN; }
        if constexpr (KB >= 2) if (nb >= 2) { load_batch(cu, c); LL_LOADS_LANDED(); count_batch(); keep_batch(std::integral_constant<int, KB - 2>{}); c += UN; }
        load_batch(cu, c); LL_LOADS_LANDED(); count_batch(); keep_batch(std::integral_constant<int, KB - 1>{});
    }
    if (bad) okflag = 0;
    __syncthreads();
    LL_GPHASE(8);
    constexpr int PER = LL_GRID_NC / LL_GB;         /* 16 */
    int sum = 0;
    for (int k = 0; k < PER; ++k) sum += hist[tid * (PER + 1) + k];
    int total = 0;
    int run = ll_block_exscan_n<LL_GB / 64>(sum, sc, total);
    for (int k = 0; k < PER; ++k) { const int c = hist[tid * (PER + 1) + k]; hist[tid * (PER + 1) + k] = run; gstart[tid * PER + k] = run; run += c; }
    if (tid == LL_GB - 1) gstart[LL_GRID_NC] = total;
    __syncthreads();
    LL_GPHASE(9);
    /* a batch of UN chunks into cell order; rb: int(intensity) & 0xFF, the walk's scan id */
    auto scatter_batch = [&](const float (&x)[UN], const float (&y)[UN], const float (&z)[UN], const int (&rb)[UN], const int (&bpl)[UN], const int (&bnv)[UN])
                         __attribute__((always_inline)) {
        int pos[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u)
            if (lane < bnv[u]) { const int cc = ll_cell_coord(y[u]) * LL_GRID_G + ll_cell_coord(x[u]); pos[u] = atomicAdd(&hist[LL_HI(cc)], 1); }
#pragma unroll
        for (int u = 0; u < UN; ++u)
            if (lane < bnv[u]) gpts[pos[u]] = make_float4(x[u], y[u], z[u], __int_as_float(((bpl[u] + lane) << 8) | rb[u]));   /* place < 2^24 */
    };
    auto scatter_loaded = [&]() __attribute__((always_inline)) {        /* the batch in p */
        float x[UN], y[UN], z[UN]; int rb[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) { x[u] = p[u].x; y[u] = p[u].y; z[u] = p[u].z; rb[u] = (int)p[u].w & 0xFF; }
        scatter_batch(x, y, z, rb, pl, nv);
    };
    auto scatter_kept = [&](auto J) __attribute__((always_inline)) {
        constexpr int j = decltype(J)::value;
        float x[UN], y[UN], z[UN]; int rb[UN], bpl[UN], bnv[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            x[u] = kx[j * UN + u]; y[u] = ky[j * UN + u]; z[u] = kz[j * UN + u];
            rb[u] = (int)((kr[(j * UN + u) / 4] >> (8 * (u & 3))) & 0xFFu);
            bpl[u] = kpn[j * UN + u] >> 7; bnv[u] = kpn[j * UN + u] & 127;
        }
        scatter_batch(x, y, z, rb, bpl, bnv);
    };
    if (nb > 0) {
        /* what the histogram sweep left in registers first, then the batches in front of the stash, read again, then the stash */
        scatter_kept(std::integral_constant<int, KB - 1>{});
        if constexpr (KB >= 2) if (nb >= 2) scatter_kept(std::integral_constant<int, KB - 2>{});
        if constexpr (KB >= 3) if (nb >= 3) scatter_kept(std::integral_constant<int, KB - 3>{});
        if (ckeep > cw0) {
            Cursor cu = cursor_at(cw0);
            const int nbf = (cst - cw0 + UN - 1) / UN;                   /* end-aligned with the stash's first chunk */
            for (int c = cst - nbf * UN; c < cst; c += UN) { load_batch(cu, c); LL_LOADS_LANDED(); scatter_loaded(); }
            const int ns = ckeep - cst;                                  /* <= stash <= UN: one batch, from LDS; the cursor stands at cst */
#pragma unroll
            for (int u = 0; u < UN; ++u) { pl[u] = 0; nv[u] = 0; if (u < ns) take(cu, pl[u], nv[u]); }
#pragma unroll
            for (int u = 0; u < UN; ++u) if (lane < nv[u]) p[u] = stw[u * 64 + lane];
            if (ns > 0) scatter_loaded();
        }
    }
#undef LL_HI
#undef LL_LOADS_LANDED
#undef LL_WSHR1
#undef LL_WSHL1

    LL_GPHASE(10);
    /* ---- ring tables + validity.  The tables first_ge / last_le (in places) reproduce the reference's sequential walk bounds for
     * EVERY start point iff no point lies before a point whose up-window it exceeds and none after a point whose
     * down-window it undercuts:
     *   exists j < c with ring_j > hi(ring_c)   <=>   exists value b:  first_ge[hi(b) + 1] < last_eq[b]
     *   exists j > c with ring_j < lo(ring_c)   <=>   exists value b:  last_le[lo(b) - 1]  > first_eq[b]
     * so validity is a check on the two 160-entry tables, no per-point scan. ---- */
    LL_GPHASE(11);
    __syncthreads();
    int *tab = gstart + LL_GRID_NC + 1;              /* first_ge[LL_TAB+1], last_le[LL_TAB+1], ok flag, m, one past the last place */
    /* first_ge = suffix minimum of the first places, last_le = prefix maximum of the last ones: wave 0, three
     * 64-entry chunks with shuffle scans, the running value carried between chunks */
    __shared__ int fge[LL_TAB + 1], lle[LL_TAB + 1];
    if (tid < 64) {
        constexpr int NCH = (LL_TAB + 1 + 63) / 64;
        int carry_min = pend;
        for (int ch = NCH - 1; ch >= 0; --ch) {
            const int v = ch * 64 + lane;
            int x = (v <= LL_TAB && feq[v] != INT_MAX) ? feq[v] : pend;
            x = min(x, pend);
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(x, o); if (lane + o < 64) x = min(x, t); }
            x = min(x, carry_min);
            if (v <= LL_TAB) { fge[v] = x; tab[v] = x; }
            carry_min = __shfl(x, 0);
        }
        int carry_max = -1;
        for (int ch = 0; ch < NCH; ++ch) {
            const int v = ch * 64 + lane;
            int x = (v <= LL_TAB) ? leq[v] : -1;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(x, o); if (lane >= o) x = max(x, t); }
            x = max(x, carry_max);
            if (v <= LL_TAB) { lle[v] = x; tab[LL_TAB + 1 + v] = x; }
            carry_max = __shfl(x, 63);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        bool viol = false, nonmono = false;
        for (int ch = 0; ch < NCH; ++ch) {
            const int bv = ch * 64 + lane;
            if (bv < LL_TAB && feq[bv] != INT_MAX) {
                const int hi = ll_ring_hi(bv, V.nearby), lo = ll_ring_lo(bv, V.nearby);
                const int fg = (hi + 1 > LL_TAB) ? pend : fge[max(hi + 1, 0)];
                const int ll = (lo - 1 < 0) ? -1 : lle[min(lo - 1, LL_TAB)];
                if (fg < leq[bv] || ll > feq[bv]) viol = true;
                if (fge[bv + 1] < leq[bv]) nonmono = true;           /* a point of a higher ring in front of a point of ring bv */
            }
        }
        const bool any_viol = __ballot(viol) != 0ull, any_nonmono = __ballot(nonmono) != 0ull;
        if (lane == 0) {
            /* bit 0: the tables bound the walks; bit 1: the ring values never decrease along the cloud (every cloud the extract stage
             * produces) -- then "same scan line" is rj == rc and the place window is the ring window, which is what lets k_associate
             * keep per-ring minima while it looks for the nearest neighbour */
            tab[2 * (LL_TAB + 1)] = ((okflag && !any_viol) ? 1 : 0) | ((okflag && !any_viol && !any_nonmono) ? 2 : 0);
            tab[2 * (LL_TAB + 1) + 1] = m;
            tab[2 * (LL_TAB + 1) + 2] = pend;
        }
    }
}

__global__ __launch_bounds__(LL_BLOCK, LL_ASSOC_WAVES) void k_associate(LLView V, int first, int count, int qb_corner, int qb_plane, int qpb)
{
    /* All query blocks of a scan on ONE XCD (workgroup b runs on XCD b % 8): they search the same target grid, and an XCD's 4 MB L2 is
     * private -- dealt round-robin over the XCDs, every scan's target would be fetched into all eight of them. */
    const int per = qb_corner + qb_plane;
    const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
    const int sl = (jb / per) * 8 + xcd, item = jb % per;
    if (sl >= count) return;
    const int s = first + sl;
    if (item == 0 && threadIdx.x == 0) V.assoc_tgt[s] = (s == V.carry_slot) ? -1 : s - 1;   /* whose points this slot's correspondences name from now on */
    __shared__ float4 qs[LL_BLOCK];
    __shared__ unsigned long long rtab[(LL_BLOCK / 8) * 2 * LL_ATAB_W];
    __shared__ int cellb[(LL_BLOCK / 8) * 3 * LL_RING_CELLS];
    __shared__ int tab[LL_TAB_WORDS];
    __shared__ unsigned char perm[LL_BLOCK];
    __shared__ int hist[64];
    const ScanHdr h = V.hdr[s];
    const bool ok = h.status == 0;
    if (item < qb_corner) {
        const int nq = ok ? h.n_sharp : 0;
        if (item * qpb >= nq) return;
        ll_associate_block<false>(V, s, item, qpb, V.sharp + (size_t)s * V.cap_sharp, nq, ll_target(V, s, 0),
                                  V.eq_a + (size_t)s * V.cap_sharp, V.eq_b + (size_t)s * V.cap_sharp, nullptr, qs, rtab, cellb, tab, perm, hist);
    } else {
        const int qb = item - qb_corner;
        const int nq = ok ? h.n_flat : 0;
        if (qb * qpb >= nq) return;
        ll_associate_block<true>(V, s, qb, qpb, V.flat + (size_t)s * V.cap_flat, nq, ll_target(V, s, 1),
                                       V.pq_a + (size_t)s * V.cap_flat, V.pq_b + (size_t)s * V.cap_flat,
                                       V.pq_c + (size_t)s * V.cap_flat, qs, rtab, cellb, tab, perm, hist);
    }
}

/* chunks per wave of k_build_grid's stash: what the device's LDS limit for a workgroup leaves beside the histogram and the kernel's
 * static arrays, in whole chunks per wave, at most one batch (MI355X: 160 KB - 68 KB - 4.2 KB -> 5) */
static int ll_grid_stash_chunks()
{
    static int cache[LL_MAX_DEVICES] = {0};         /* stash + 1; 0: not asked yet */
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= LL_MAX_DEVICES) dev = 0;
    if (cache[dev] == 0) {
        int per_block = 0, per_cu = 0;
        hipFuncAttributes fa;
        if (hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) per_block = 0;
        if (hipDeviceGetAttribute(&per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess) per_cu = 0;
        long long room = -1;
        if (hipFuncGetAttributes(&fa, (const void *)k_build_grid) == hipSuccess)
            room = (long long)(per_block > per_cu ? per_block : per_cu) - (long long)fa.sharedSizeBytes - (long long)LL_GRID_HIST_BYTES;
        (void)hipGetLastError();
        const long long per_wave = room / (long long)((LL_GB / 64) * 64 * sizeof(float4));
        cache[dev] = 1 + (int)(per_wave < 0 ? 0 : per_wave > LL_GRID_UN ? LL_GRID_UN : per_wave);
    }
    return cache[dev] - 1;
}

void ll_launch_build_grid(const LLView &V, int first, int count, int carry, hipStream_t st, LLProfiler *prof)
{
    static size_t attr_bytes[LL_MAX_DEVICES] = {0};   /* 68 KiB histogram + the stashes + static LDS exceed the default dynamic-LDS limit */
    const int stash = ll_grid_stash_chunks();
    const size_t lds = ll_grid_lds_bytes(stash);
    ll_ensure_dynamic_lds(k_build_grid, lds, attr_bytes);
    ll_prof_mark(prof, LL_K_GRID, st);
    hipLaunchKernelGGL(k_build_grid, dim3(2 * (carry ? 1 : count)), dim3(LL_GB), lds, st, V, first, carry ? 1 : count, carry, stash);
    ll_prof_mark(prof, LL_K_END, st);
}

void ll_launch_associate(const LLView &V, int first, int count, hipStream_t st, LLProfiler *prof)
{
    /* a node-style call (one scan pair) would put 9 workgroups of 8 sequential passes on a 256-CU chip: 217 us of dependent
     * loads; 32 queries per workgroup (one pass) spread the same work over 72 workgroups */
#ifdef LL_ASSOC_QPB
    const int qpb = (count <= 16) ? 32 : LL_ASSOC_QPB;         /* A/B builds (tools/make_ab_variant.sh) */
#else
    const int qpb = (count <= 16) ? 32 : LL_BLOCK;
#endif
    const int qbc = (V.cap_sharp + qpb - 1) / qpb, qbp = (V.cap_flat + qpb - 1) / qpb;
    ll_prof_mark(prof, LL_K_ASSOCIATE, st);
    hipLaunchKernelGGL(k_associate, dim3(8 * (qbc + qbp) * ((count + 7) / 8)), dim3(LL_BLOCK), 0, st, V, first, count, qbc, qbp, qpb);
    ll_prof_mark(prof, LL_K_END, st);
}
