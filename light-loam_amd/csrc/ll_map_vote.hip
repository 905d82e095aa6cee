/*
 * ll_map_vote.hip -- the graph-based correspondence vote of the MAPPING stage: laserMapping.cpp's own
 * graph_based_correspondence_vote_simple (:836-1030), the Corre_Match it is fed (:1843-1850, :1993-2003, :2026) and the gate that
 * hands the selected blocks to the problem (:2057-2072).  The reference has the call commented out; ll_map_set_vote and its
 * relatives switch it on per map, off is the default and changes nothing by a bit.
 *
 * Input: one correspondence per plane block that passed planeValid, in stack order -- the compacted plane list as k_map_compact /
 * k_cms_compact leave it.  src = the raw stack point (lidar frame), tgt = the float centroid of its five neighbours, which the
 * plane fit stores per stack point when the view's ctr is set (ll_map_search.h).
 *   k_map_vote          one workgroup per (view, region): 20 regions (:841) of n / 20 candidates, the last one takes the remainder
 *                       (:884-893).  The region's records are staged once in LDS (28 B each: src, tgt, a count), every unordered
 *                       pair is tested once by the circular-offset schedule of ll_vote_core (ll_vote.h), counts are LDS atomics.
 *                       The pair test is (double)expf(-gap^2) < 0.95 as the bit-exact threshold on the gap of ll_exact_math.h,
 *                       decided from hardware square roots except inside the band where only the exact roots can tell.
 *                       Selection (:965-1027, corner_case = true at :2059): (float)count < 0.75f * (float)m, strict.
 *   k_map_vote_compact  one workgroup per view: keeps the candidates (stack index, count, flag, their number) for download and
 *                       compacts src[1], fn, fd in place to the selected blocks, chunk by chunk -- a chunk is read before it is
 *                       written and positions only move down -- then writes counts[1].  The solve kernels read what they always read.
 * Two decisions: (1) with the vote on, the plane blocks of the solve are the selected ones INSTEAD of all of them -- the intent of the
 * commented gate at :2027-2032; the literal text would add the selected blocks a second time on top of :2033.  (2) The selected
 * blocks keep stack order, as the odometry vote keeps correspondence order; the reference's order (descending sort, walked from the
 * back) only permutes residual blocks.  The weight is 1 (LidarPlaneNormFactor takes none); edge blocks are never voted.
 * No kernel here waits on another workgroup; nothing here synchronises with the host.
 */
#include "ll_common.h"
#include "ll_exact_math.h"

extern __shared__ __attribute__((aligned(16))) unsigned char ll_mvsm[];

#define LL_MVT 256            /* threads of both kernels: a region of a frame holds 100 - 400 candidates */

__global__ __launch_bounds__(LL_MVT) void k_map_vote(const LLMapView *views, int cap_region)
{
    const LLMapView &M = views[blockIdx.x / LL_MAP_VOTE_REGIONS];
    if (!M.ctr) return;
    const int rg = blockIdx.x % LL_MAP_VOTE_REGIONS;
    const int n = M.counts[1];
    const int chunk = n / LL_MAP_VOTE_REGIONS;                                      /* :884-893 */
    const int b0 = chunk * rg, b1 = (rg == LL_MAP_VOTE_REGIONS - 1) ? n : chunk * (rg + 1);
    const int m = b1 - b0;
    if (m <= 0) return;
    if (m > cap_region) {        /* the launcher sizes the LDS from the stack sizes, which bound n: never taken; if it were, nothing is dropped and the count says so */
        for (int i = threadIdx.x; i < m; i += LL_MVT) { M.v_count[b0 + i] = -1; M.v_sel[b0 + i] = 1; }
        return;
    }
    float *S3 = (float *)ll_mvsm;                                                   /* [m][6]: src xyz, tgt xyz */
    int *cntL = (int *)(S3 + 6 * (size_t)m);                                        /* [m] */
    for (int i = threadIdx.x; i < m; i += LL_MVT) {
        const int s = M.src[1][b0 + i];
        const float4 a = M.stk[1][s];                                               /* cor.src = laserCloudSurfStack->points[i] (:1995) */
        const float *c = M.ctr + (size_t)s * 3;                                     /* cor.tgt = (cx, cy, cz) (:1996-2000) */
        S3[6 * i] = a.x; S3[6 * i + 1] = a.y; S3[6 * i + 2] = a.z;
        S3[6 * i + 3] = c[0]; S3[6 * i + 4] = c[1]; S3[6 * i + 5] = c[2];
        cntL[i] = 0;
    }
    __syncthreads();
    /* every unordered pair once (:918-944): entry i takes the partners at circular offsets 1 .. (m - 1) / 2, and for even m the
     * lower half also takes offset m / 2 */
    const int half = (m - 1) / 2;
    const float gT = ll_u2f(LL_MAP_VOTE_GAP_BITS);
    for (int i = threadIdx.x; i < m; i += LL_MVT) {
        const float ax = S3[6 * i], ay = S3[6 * i + 1], az = S3[6 * i + 2];
        const float bx = S3[6 * i + 3], by = S3[6 * i + 4], bz = S3[6 * i + 5];
        const int nd = half + (((m & 1) == 0 && i < m / 2) ? 1 : 0);
        int cnt = 0, j = i;
        for (int d = 1; d <= nd; ++d) {
            ++j; if (j >= m) j -= m;
            /* Distance() (:250): f32 sqrt of dx*dx + dy*dy + dz*dz; squares, so (i, j) and (j, i) are the same test bit for bit */
            const float2 *pj = (const float2 *)(S3 + 6 * j);
            const float2 p0 = pj[0], p1 = pj[1], p2 = pj[2];
            float dx = ax - p0.x, dy = ay - p0.y, dz = az - p1.x;
            const float a2 = dx * dx + dy * dy + dz * dz;
            dx = bx - p1.y; dy = by - p2.x; dz = bz - p2.y;
            const float b2 = dx * dx + dy * dy + dz * dz;
            /* gap >= g_T on correctly rounded roots is the reference's test.  The hardware root (v_sqrt_f32, ~1 ulp) decides it
             * unless the approximate gap lies within (s1 + s2) * 2^-20 of g_T -- more than three times what two approximate roots
             * and the roundings of the subtractions can move it; the band does not depend on the threshold -- and only those
             * pairs, and the non-finite ones, take the exact roots */
            const float s1a = __builtin_amdgcn_sqrtf(a2), s2a = __builtin_amdgcn_sqrtf(b2);
            const float ga = fabsf(s1a - s2a), e2 = (s1a + s2a) * 9.5367431640625e-07f;
            bool inc = ga >= gT + e2;
            if (!inc && !(ga <= gT - e2)) {
                const float s1 = sqrtf(a2), s2 = sqrtf(b2);
                inc = ll_map_vote_incompatible_gap(fabsf(s1 - s2));
            }
            if (inc) { ++cnt; atomicAdd(&cntL[j], 1); }
        }
        if (cnt) atomicAdd(&cntL[i], cnt);
    }
    __syncthreads();
    const float num_selected = 0.75f * (float)m;                                    /* :969-970 */
    for (int i = threadIdx.x; i < m; i += LL_MVT) {
        const int cnt = cntL[i];
        M.v_count[b0 + i] = cnt;
        M.v_sel[b0 + i] = (unsigned char)((float)cnt < num_selected);               /* :996, strict */
    }
}

__global__ __launch_bounds__(LL_MVT) void k_map_vote_compact(const LLMapView *views)
{
    __shared__ int sc[LL_MVT / 64];
    const LLMapView &M = views[blockIdx.x];
    if (!M.ctr) return;
    const int tid = threadIdx.x;
    const int n = M.counts[1];
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += LL_MVT) {
        const int i = c0 + tid;
        int s = 0; double v[4] = {0.0, 0.0, 0.0, 0.0}; bool keep = false;
        if (i < n) {
            s = M.src[1][i]; keep = M.v_sel[i] != 0;
            for (int k = 0; k < 3; ++k) v[k] = M.fn[(size_t)i * 3 + k];
            v[3] = M.fd[i];
            M.v_src[i] = s;
        }
        int total;
        const int pos = base + ll_block_exscan_n<LL_MVT / 64>(keep ? 1 : 0, sc, total);   /* its barriers: every read of the chunk is done */
        if (keep) {                                                                  /* pos <= i: never into a chunk not yet read */
            M.src[1][pos] = s;
            for (int k = 0; k < 3; ++k) M.fn[(size_t)pos * 3 + k] = v[k];
            M.fd[pos] = v[3];
        }
        base += total;
    }
    if (tid == 0) { M.v_n[0] = n; M.counts[1] = base; }
}

static void ll_map_vote_launch(const LLMapView *d_views, int n_views, int max_stk, bool compact, hipStream_t st)
{
    if (n_views <= 0) return;
    const int cap_region = ll_map_vote_region_max(max_stk > 0 ? max_stk : 0);
    const size_t lds = (size_t)cap_region * 28;
    static size_t attr_bytes[LL_MAX_DEVICES] = {0};
    ll_ensure_dynamic_lds(k_map_vote, lds, attr_bytes);
    hipLaunchKernelGGL(k_map_vote, dim3((unsigned)n_views * LL_MAP_VOTE_REGIONS), dim3(LL_MVT), lds, st, d_views, cap_region);
    if (compact) hipLaunchKernelGGL(k_map_vote_compact, dim3((unsigned)n_views), dim3(LL_MVT), 0, st, d_views);
}

void ll_map_launch_vote(const LLMapView *d_views, int n_views, int max_stk, hipStream_t st) { ll_map_vote_launch(d_views, n_views, max_stk, true, st); }
void ll_map_launch_vote_only(const LLMapView *d_views, int n_views, int max_stk, hipStream_t st) { ll_map_vote_launch(d_views, n_views, max_stk, false, st); }
