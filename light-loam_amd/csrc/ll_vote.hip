/*
 * ll_vote.hip -- correspondence compaction + a8: graph_based_correspondence_vote_simple.
 * Replaces laserOdometry.cpp:153-342 (call site :796) of /root/reference, plus the push_back order of the
 * correspondence lists (:574-585, :745-757).
 *
 * One workgroup per scan pair.  Per-query association results are compacted in query order (the order the
 * reference appends them).  The vote is the reference's dense all-pairs test inside each of 10 (planes) or 5
 * (corners) contiguous regions: every pair (i, j) of a region with | |src_i-src_j| - |tgt_i-tgt_j| |^2 >= T counts for both,
 * where "std::exp(-gap^2) < 0.96f" is replaced by the bit-exact threshold of ll_exact_math.h.  src/tgt points are
 * staged once in LDS and broadcast-read.  Selection: count <= 0.9f*m, weight 5 if count <= 50 else 1 (:299-322).
 * Output is per correspondence (count, selected, weight); the reference's output ORDER (ascending count, std::sort
 * ties unspecified) only permutes residual blocks and is reproduced on the host side where a caller needs it
 * (include/lightloam_host.hpp runs the same std::sort on the counts).
 */
#include "ll_vote.h"

__global__ __launch_bounds__(LL_VT) void k_vote(LLView V, int first, int count, int enable)
{
    if ((int)blockIdx.x >= count) return;
    const int s = first + blockIdx.x;
    const int tid = threadIdx.x;
    __shared__ int sc[LL_VT / 64 + 1];
    __shared__ int nsel_sh;
    const ScanHdr h = V.hdr[s];
    const bool ok = h.status == 0;
    const int ns = ok ? h.n_sharp : 0, nf = ok ? h.n_flat : 0;
    const float4 *corner, *surf; int mc, ms;
    ll_targets(V, s, corner, mc, surf, ms);

    /* edges (:574-617) */
    const int *eqa = V.eq_a + (size_t)s * V.cap_sharp, *eqb = V.eq_b + (size_t)s * V.cap_sharp;
    int *es = V.e_src + (size_t)s * V.cap_sharp, *ea = V.e_a + (size_t)s * V.cap_sharp, *eb = V.e_b + (size_t)s * V.cap_sharp;
    const int n_e = ll_block_compact<LL_VT>(ns, sc, [&](int i, int pos) { es[pos] = i; ea[pos] = eqa[i]; eb[pos] = eqb[i]; }, eqa);
    /* planes (:745-790) */
    const int *pqa = V.pq_a + (size_t)s * V.cap_flat, *pqb = V.pq_b + (size_t)s * V.cap_flat, *pqc = V.pq_c + (size_t)s * V.cap_flat;
    int *ps = V.p_src + (size_t)s * V.cap_flat, *pa = V.p_a + (size_t)s * V.cap_flat, *pb = V.p_b + (size_t)s * V.cap_flat, *pc = V.p_c + (size_t)s * V.cap_flat;
    const int n_p = ll_block_compact<LL_VT>(nf, sc, [&](int i, int pos) { ps[pos] = i; pa[pos] = pqa[i]; pb[pos] = pqb[i]; pc[pos] = pqc[i]; }, pqa);

    /* stage Corre_Match.src (raw current point, :753) and .tgt (closest target point, :754) */
    float *S3 = (float *)ll_vsm;                 /* [n_p][6]: src xyz, tgt xyz */
    float *T3 = S3 + 3 * (size_t)V.cap_flat;     /* S3 + 6 * cap_flat = T3 + 3 * cap_flat: the counts */
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
}

/* the free function's own signature: caller-supplied correspondences (src / tgt points), 5 or 10 regions */
__global__ __launch_bounds__(LL_BLOCK) void k_vote_points(const float4 *src, const float4 *tgt, int n, int regions,
                                                          int *vc, uint8_t *vs, float *vw)
{
    float *S3 = (float *)ll_vsm, *T3 = S3 + 3 * (size_t)n;
    for (int i = threadIdx.x; i < n; i += LL_BLOCK) {
        const float4 a = src[i], b = tgt[i];
        S3[6 * i] = a.x; S3[6 * i + 1] = a.y; S3[6 * i + 2] = a.z;
        S3[6 * i + 3] = b.x; S3[6 * i + 4] = b.y; S3[6 * i + 5] = b.z;
    }
    __syncthreads();
    (void)ll_vote_core<LL_BLOCK>(S3, T3, n, regions, 1, vc, vs, vw, (int *)(T3 + 3 * (size_t)n));
}

void ll_launch_vote(const LLView &V, int first, int count, int enable, hipStream_t st, LLProfiler *prof)
{
    const size_t lds = (size_t)V.cap_flat * 28;                   /* src + tgt triples + one count per correspondence */
    static size_t attr_bytes[LL_MAX_DEVICES] = {0};
    ll_ensure_dynamic_lds(k_vote, lds, attr_bytes);
    ll_prof_mark(prof, LL_K_VOTE, st);
    hipLaunchKernelGGL(k_vote, dim3(count), dim3(LL_VT), lds, st, V, first, count, enable);
    ll_prof_mark(prof, LL_K_END, st);
}

void ll_launch_vote_points(const float4 *src, const float4 *tgt, int n, int regions, int *vc, uint8_t *vs, float *vw, hipStream_t st)
{
    const size_t lds = (size_t)n * 28 + 16;
    static size_t attr_bytes[LL_MAX_DEVICES] = {0};
    ll_ensure_dynamic_lds(k_vote_points, lds, attr_bytes);
    hipLaunchKernelGGL(k_vote_points, dim3(1), dim3(LL_BLOCK), lds, st, src, tgt, n, regions, vc, vs, vw);
}
