/*
 * ll_sequences.hip -- the kernels of ll_odometry_sequences (ll_api.hip): laserOdometry's frame loop for S independent sequences side
 * by side.  The frames sit in a ring of rows, one row = S contiguous slots; a row of all sequences advances per launch pair:
 *   k_associate_rows   k_associate over the row's slots, the target of slot s being row_pred[s] (the same sequence's previous frame)
 *   k_vote_lm_rows     k_vote's body, then k_lm_solve's, on one 512-thread workgroup per slot; on the last outer iteration the solved
 *                      pose is also the warm start of the successor row's slot (laserOdometry.cpp:61-65)
 * Only slots whose row_mode bit 0 is set run; bit 1 is their vote switch (frame index > 5, :794).  row_pred / row_mode are written per
 * call by ll_api.hip's setup kernel.
 *
 * The per-query search (ll_associate_block, ll_associate.h), the compaction and vote (ll_vote.h), the normal equations (ll_neq.h) and
 * the trust-region steps (ll_lm_step.h) are the functions the single-sequence kernels call.  The few lines that glue them into a
 * kernel are repeated here instead of being moved into shared functions: every such refactoring tried changed the register
 * allocation of k_associate / k_vote / k_lm_solve, and those kernels keep their code.  Kernels in their own translation unit for the
 * same reason: a second caller of ll_associate_block in ll_associate.hip changes k_associate's code too.
 */
#include "ll_associate.h"
#include "ll_vote.h"
#include "ll_neq.h"
#include "ll_lm_step.h"

__global__ __launch_bounds__(LL_BLOCK, LL_ASSOC_WAVES) void k_associate_rows(LLView V, int first, int count, int qb_corner, int qb_plane, int qpb)
{
    /* the dealing of k_associate: all query blocks of a slot on one XCD */
    const int per = qb_corner + qb_plane;
    const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
    const int sl = (jb / per) * 8 + xcd, item = jb % per;
    if (sl >= count) return;
    const int s = first + sl;
    if ((V.row_mode[s] & 1) == 0) return;                 /* not run in this call: nothing of the slot is written */
    const int t = V.row_pred[s];
    if (item == 0 && threadIdx.x == 0) V.assoc_tgt[s] = t;  /* vote, factors and solve read the target from here */
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
        ll_associate_block<false>(V, s, item, qpb, V.sharp + (size_t)s * V.cap_sharp, nq, ll_target_row(V, t, 0),
                                  V.eq_a + (size_t)s * V.cap_sharp, V.eq_b + (size_t)s * V.cap_sharp, nullptr, qs, rtab, cellb, tab, perm, hist);
    } else {
        const int qb = item - qb_corner;
        const int nq = ok ? h.n_flat : 0;
        if (qb * qpb >= nq) return;
        ll_associate_block<true>(V, s, qb, qpb, V.flat + (size_t)s * V.cap_flat, nq, ll_target_row(V, t, 1),
                                 V.pq_a + (size_t)s * V.cap_flat, V.pq_b + (size_t)s * V.cap_flat,
                                 V.pq_c + (size_t)s * V.cap_flat, qs, rtab, cellb, tab, perm, hist);
    }
}

/* One row after its association.  k_vote and k_lm_solve both run 512 threads (LL_VT, LL_LM_THREADS): the compaction, the vote and
 * the 512-way f64 sums of ll_neq_eval are those of the two launches of ll_odometry_frames, so the poses agree bit for bit.  The vote's
 * records take the dynamic LDS (cap_flat x 28 B), the solve its static arrays.  succ_first >= 0 (last outer iteration of a row with a
 * successor in the call): the solved pose is also written to slot succ_first + blockIdx.x when that slot runs. */
static_assert(LL_VT == LL_LM_THREADS, "the fused vote + solve runs both bodies on one workgroup size");
template <bool DIST>
__global__ __launch_bounds__(LL_LM_THREADS) void k_vote_lm_rows(LLView V, int first, int count, int succ_first, LLLmOpt o)
{
    if ((int)blockIdx.x >= count) return;
    const int s = first + blockIdx.x;
    const int mode = V.row_mode[s];
    if ((mode & 1) == 0) return;
    const int enable = (mode >> 1) & 1;
    const int tid = threadIdx.x;

    /* ---- k_vote (ll_vote.hip) */
    {
        __shared__ int sc[LL_VT / 64 + 1];
        __shared__ int nsel_sh;
        const ScanHdr h = V.hdr[s];
        const bool ok = h.status == 0;
        const int ns = ok ? h.n_sharp : 0, nf = ok ? h.n_flat : 0;
        const float4 *corner, *surf; int mc, ms;
        ll_targets(V, s, corner, mc, surf, ms);
        const int *eqa = V.eq_a + (size_t)s * V.cap_sharp, *eqb = V.eq_b + (size_t)s * V.cap_sharp;
        int *es = V.e_src + (size_t)s * V.cap_sharp, *ea = V.e_a + (size_t)s * V.cap_sharp, *eb = V.e_b + (size_t)s * V.cap_sharp;
        const int n_e = ll_block_compact<LL_VT>(ns, sc, [&](int i, int pos) { es[pos] = i; ea[pos] = eqa[i]; eb[pos] = eqb[i]; }, eqa);
        const int *pqa = V.pq_a + (size_t)s * V.cap_flat, *pqb = V.pq_b + (size_t)s * V.cap_flat, *pqc = V.pq_c + (size_t)s * V.cap_flat;
        int *ps = V.p_src + (size_t)s * V.cap_flat, *pa = V.p_a + (size_t)s * V.cap_flat, *pb = V.p_b + (size_t)s * V.cap_flat, *pc = V.p_c + (size_t)s * V.cap_flat;
        const int n_p = ll_block_compact<LL_VT>(nf, sc, [&](int i, int pos) { ps[pos] = i; pa[pos] = pqa[i]; pb[pos] = pqb[i]; pc[pos] = pqc[i]; }, pqa);
        float *S3 = (float *)ll_vsm;
        float *T3 = S3 + 3 * (size_t)V.cap_flat;
        const float4 *flat = V.flat + (size_t)s * V.cap_flat;
        if (tid == 0) nsel_sh = 0;
        __syncthreads();
        for (int i = tid; i < n_p; i += LL_VT) {
            const float4 a = flat[ps[i]], b = surf[pa[i]];
            S3[6 * i] = a.x; S3[6 * i + 1] = a.y; S3[6 * i + 2] = a.z;
            S3[6 * i + 3] = b.x; S3[6 * i + 4] = b.y; S3[6 * i + 5] = b.z;
        }
        __syncthreads();
        const int my_sel = ll_vote_core<LL_VT>(S3, T3, n_p, 10 /* plane case (:186-187) */, enable,
                                               V.v_count + (size_t)s * V.cap_flat, V.v_sel + (size_t)s * V.cap_flat, V.v_w + (size_t)s * V.cap_flat,
                                               (int *)(T3 + 3 * (size_t)V.cap_flat));
        if (my_sel) atomicAdd(&nsel_sh, my_sel);
        __syncthreads();
        if (tid == 0) {
            PairHdr p; p.n_edge = n_e; p.n_plane = n_p; p.n_plane_sel = nsel_sh; p.target_slot = ll_target_slot(V, s);
            V.pair[s] = p;
        }
        __syncthreads();                               /* the pair header and the compacted lists: read by every thread of the solve */
    }

    /* ---- k_lm_solve (ll_factors.hip) */
    __shared__ double red[LL_LM_THREADS / 64][LL_NACC];
    __shared__ double sp[7], sneq[LL_NEQ_STRIDE], sL[LL_LM_STRIDE];
    if (tid < 7) sp[tid] = V.pose[(size_t)s * 7 + tid];
    for (int k = tid; k < LL_LM_STRIDE; k += LL_LM_THREADS) sL[k] = 0.0;
    __syncthreads();
    ll_neq_eval<LL_LM_THREADS, DIST>(V, s, sp, sneq, red);
    if (tid == 0) ll_lm_begin_one(sL, sneq, sp, o);
    for (int it = 0; it < o.max_num_iterations; ++it) {
        if (tid == 0) ll_lm_propose_one(sL, sp, o);
        __syncthreads();
        ll_neq_eval<LL_LM_THREADS, DIST>(V, s, sp, sneq, red);
        if (tid == 0) ll_lm_accept_one(sL, sneq, sp, o);
    }
    __syncthreads();
    if (tid < 7) V.pose[(size_t)s * 7 + tid] = sp[tid];
    for (int k = tid; k < LL_NEQ_STRIDE; k += LL_LM_THREADS) V.neq[(size_t)s * LL_NEQ_STRIDE + k] = sneq[k];
    for (int k = tid; k < LL_LM_STRIDE; k += LL_LM_THREADS) V.lm[(size_t)s * LL_LM_STRIDE + k] = sL[k];

    /* ---- the warm start of the successor row (:61-65) */
    if (succ_first >= 0 && tid < 7) {
        const int u = succ_first + blockIdx.x;
        if (V.row_mode[u] & 1) V.pose[(size_t)u * 7 + tid] = sp[tid];
    }
}

void ll_launch_associate_rows(const LLView &V, int first, int count, hipStream_t st, LLProfiler *prof)
{
    /* a row holds one scan per sequence: the query-block size follows the number of sequences as ll_launch_associate's follows count */
    const int qpb = (count <= 16) ? 32 : LL_BLOCK;
    const int qbc = (V.cap_sharp + qpb - 1) / qpb, qbp = (V.cap_flat + qpb - 1) / qpb;
    ll_prof_mark(prof, LL_K_ASSOCIATE, st);
    hipLaunchKernelGGL(k_associate_rows, dim3(8 * (qbc + qbp) * ((count + 7) / 8)), dim3(LL_BLOCK), 0, st, V, first, count, qbc, qbp, qpb);
    ll_prof_mark(prof, LL_K_END, st);
}

void ll_launch_vote_lm_rows(const LLView &V, int first, int count, int succ_first, const LLLmOpt &o, hipStream_t st, LLProfiler *prof)
{
    const size_t lds = (size_t)V.cap_flat * 28;        /* as ll_launch_vote: src + tgt triples + one count per correspondence */
    static size_t attr_bytes[2][LL_MAX_DEVICES] = {{0}, {0}};
    ll_prof_mark(prof, LL_K_VOTE, st);
    if (V.distortion) {
        ll_ensure_dynamic_lds(k_vote_lm_rows<true>, lds, attr_bytes[1]);
        hipLaunchKernelGGL(k_vote_lm_rows<true>, dim3(count), dim3(LL_LM_THREADS), lds, st, V, first, count, succ_first, o);
    } else {
        ll_ensure_dynamic_lds(k_vote_lm_rows<false>, lds, attr_bytes[0]);
        hipLaunchKernelGGL(k_vote_lm_rows<false>, dim3(count), dim3(LL_LM_THREADS), lds, st, V, first, count, succ_first, o);
    }
    ll_prof_mark(prof, LL_K_END, st);
}
