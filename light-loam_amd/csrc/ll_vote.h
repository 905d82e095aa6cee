/*
 * ll_vote.h -- the device helpers of the correspondence compaction + vote (ll_vote.hip), shared with the fused vote + solve of
 * ll_odometry_sequences (k_vote_lm_rows, ll_sequences.hip).
 */
#pragma once
#include "ll_common.h"

extern __shared__ __attribute__((aligned(16))) unsigned char ll_vsm[];

/* stable compaction of valid_src[0..n) >= 0 by one workgroup; emit(i, pos) for every kept i; returns the total */
template <int NT, typename F>
__device__ __forceinline__ int ll_block_compact(int n, int *sc, F emit, const int *valid_src)
{
    const int tid = threadIdx.x;
    const int per = (n + NT - 1) / NT;
    const int a0 = min(n, tid * per), a1 = min(n, a0 + per);
    int c = 0;
    for (int i = a0; i < a1; ++i) c += valid_src[i] >= 0;
    int total = 0;
    int pos = ll_block_exscan_n<NT / 64>(c, sc, total);
    for (int i = a0; i < a1; ++i) if (valid_src[i] >= 0) emit(i, pos++);
    __syncthreads();
    return total;
}

/* the vote proper on LDS-staged records S3[6 * i .. 6 * i + 5] = (src xyz, tgt xyz) of correspondence i (T3 = the end of the
 * records); returns this thread's number of selected entries.
 * Every unordered pair of a region is evaluated ONCE, like the reference's i < j loop (:228-252): entry i of a region of m
 * takes the partners at circular offsets 1 .. (m - 1) / 2 (and, for even m, the lower half takes offset m / 2), which
 * gives every lane the same trip count; an incompatible pair bumps the entry's own register count and the partner's
 * count in LDS (cntL, n_p ints, zeroed here).  Counts are integers, so the summation order does not matter. */
template <int NT>
__device__ __forceinline__ int ll_vote_core(const float *S3, const float *T3, int n_p, int number_of_region, int enable,
                                            int *vc, uint8_t *vs, float *vw, int *cntL)
{
    const int chunk = n_p / number_of_region;                     /* cor_size_all / number_of_region (:202) */
    for (int i = threadIdx.x; i < n_p; i += NT) cntL[i] = 0;
    __syncthreads();
    if (enable) {
        for (int i = threadIdx.x; i < n_p; i += NT) {
            const int rg = (chunk > 0) ? min(i / chunk, number_of_region - 1) : number_of_region - 1;
            const int b0 = chunk * rg, b1 = (rg == number_of_region - 1) ? n_p : chunk * (rg + 1);
            const int m = b1 - b0;
            const float ax = S3[6 * i], ay = S3[6 * i + 1], az = S3[6 * i + 2];
            const float bx = S3[6 * i + 3], by = S3[6 * i + 4], bz = S3[6 * i + 5];
            const int half = (m - 1) / 2;
            const int nd = half + (((m & 1) == 0 && (i - b0) < m / 2) ? 1 : 0);        /* even m: offset m / 2 once per pair */
            int cnt = 0;
            int j = i;
            for (int d = 1; d <= nd; ++d) {
                ++j; if (j >= b1) j -= m;
                /* Distance() (:153-162): f32 sqrt of dx*dx + dy*dy + dz*dz; the squares make the operand order irrelevant
                 * bit-for-bit, so (i, j) and (j, i) are the same test */
                const float2 *pj = (const float2 *)(S3 + 6 * j);                  /* one record: three 8-byte reads */
                const float2 p0 = pj[0], p1 = pj[1], p2 = pj[2];
                float dx = ax - p0.x, dy = ay - p0.y, dz = az - p1.x;
                const float a2 = dx * dx + dy * dy + dz * dz;
                dx = bx - p1.y; dy = by - p2.x; dz = bz - p2.y;
                const float b2 = dx * dx + dy * dy + dz * dz;
                /* The reference's test is gap >= g_T on correctly rounded square roots (ll_vote_incompatible_gap).  The
                 * hardware square root (v_sqrt_f32, ~1 ulp) decides it unless the approximate gap lies within
                 * (s1 + s2) * 2^-20 of g_T -- more than three times what two approximate roots (a few ulp each) and the
                 * roundings of the two subtractions can move it -- and only those pairs take the exact roots. */
                const float s1a = __builtin_amdgcn_sqrtf(a2), s2a = __builtin_amdgcn_sqrtf(b2);
                const float ga = fabsf(s1a - s2a), e2 = (s1a + s2a) * 9.5367431640625e-07f;
                const float gT = ll_u2f(LL_VOTE_GAP_BITS);
                bool inc = ga >= gT + e2;
                if (!inc && !(ga <= gT - e2)) {                                    /* too close to call (or not finite) */
                    const float s1 = sqrtf(a2), s2 = sqrtf(b2);
                    inc = ll_vote_incompatible_gap(fabsf(s1 - s2));
                }
                if (inc) { ++cnt; atomicAdd(&cntL[j], 1); }
            }
            if (cnt) atomicAdd(&cntL[i], cnt);
        }
    }
    __syncthreads();
    int my_sel = 0;
    for (int i = threadIdx.x; i < n_p; i += NT) {
        int cnt = 0, sel = 1; float w = 1.0f;
        if (enable) {
            const int rg = (chunk > 0) ? min(i / chunk, number_of_region - 1) : number_of_region - 1;
            const int b0 = chunk * rg, b1 = (rg == number_of_region - 1) ? n_p : chunk * (rg + 1);
            cnt = cntL[i];
            const float num_selected = 0.90f * (float)(b1 - b0);                 /* :299-300 */
            sel = !((float)cnt > num_selected);                                   /* :312 */
            w = ((float)cnt <= 50.0f) ? 5.0f : 1.0f;                              /* :317-322 */
        }
        vc[i] = cnt; vs[i] = (uint8_t)sel; vw[i] = w;
        my_sel += sel;
    }
    return my_sel;
}

/* LL_VT threads: the all-pairs loop is the serial work of a thread (72 k pair tests per scan pair: ~280 each with 256 threads);
 * 256 / 512 / 1024 threads: 0.80 / 0.63 / 1.14 ms per 8192 scan pairs */
#ifndef LL_VT
#define LL_VT 512
#endif
