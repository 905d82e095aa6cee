/*
 * ll_map_search.h -- the per-stack-point search and fit of the mapping stage (ll_mapping.hip): pointAssociateToMap, the exact
 * five nearest over the 27 grid cells, the line / plane fit.  Shared by k_map_knn (ll_mapping.hip) and the batched search of
 * ll_cubemaps.hip, which runs the same code per sequence.
 */
#pragma once
#include "ll_common.h"
#include <limits.h>

/* order-preserving float <-> int for atomicMin / atomicMax */
__device__ __forceinline__ int ll_f2ord(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }

/* ---- 3 x 3 symmetric eigen-decomposition, cyclic Jacobi ---- */
__device__ __forceinline__ void ll_sym_eig3(const double Ain[3][3], double w[3], double V[3][3])
{
    double A[3][3], Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] = Ain[i][j];
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (off <= 1e-32 * diag || off == 0.0) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - sn * akq; A[k][q] = sn * akp + c * akq; }
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - sn * aqk; A[q][k] = sn * apk + c * aqk; }
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double qkp = Q[k][p], qkq = Q[k][q]; Q[k][p] = c * qkp - sn * qkq; Q[k][q] = sn * qkp + c * qkq; }
            }
    }
    /* ascending eigenvalues: bubble the three diagonal entries, columns follow */
    double d[3] = {A[0][0], A[1][1], A[2][2]};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2 - i; ++j)
            if (d[j] > d[j + 1]) {
                const double td = d[j]; d[j] = d[j + 1]; d[j + 1] = td;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double tq = Q[k][j]; Q[k][j] = Q[k][j + 1]; Q[k][j + 1] = tq; }
            }
    for (int k = 0; k < 3; ++k) { w[k] = d[k]; for (int i = 0; i < 3; ++i) V[i][k] = Q[i][k]; }
}

/* ---- 5 x 3 least squares by Householder QR with column pivoting ---- */
__device__ __forceinline__ void ll_qr_solve_5x3(double A[5][3], double b[5], double x[3])
{
    int perm[3] = {0, 1, 2};
    double maxn2 = 0.0;
    for (int j = 0; j < 3; ++j) { double n2 = 0.0; for (int i = 0; i < 5; ++i) n2 += A[i][j] * A[i][j]; if (n2 > maxn2) maxn2 = n2; }
    const double thr = maxn2 * (2.220446049250313e-16 * 2.220446049250313e-16) / 5.0;
    int rank = 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= rank) break;
        int piv = k; double best = -1.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j < k) continue;
            double n2 = 0.0;
            for (int i = k; i < 5; ++i) n2 += A[i][j] * A[i][j];
            if (n2 > best) { best = n2; piv = j; }
        }
        if (best < thr) { rank = k; break; }
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j == piv && piv != k) {
                for (int i = 0; i < 5; ++i) { const double tmp = A[i][k]; A[i][k] = A[i][j]; A[i][j] = tmp; }
                const int tp = perm[k]; perm[k] = perm[j]; perm[j] = tp;
            }
        double tail = 0.0;
        for (int i = k + 1; i < 5; ++i) tail += A[i][k] * A[i][k];
        const double c0 = A[k][k];
        double tau, beta, v[5];
        if (tail <= 2.2250738585072014e-308) { tau = 0.0; beta = c0; for (int i = 0; i < 5; ++i) v[i] = 0.0; }
        else {
            beta = sqrt(c0 * c0 + tail); if (c0 >= 0.0) beta = -beta;
            for (int i = 0; i < 5; ++i) v[i] = (i > k) ? A[i][k] / (c0 - beta) : 0.0;
            tau = (beta - c0) / beta;
        }
        v[k] = 1.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j <= k) continue;
            double d = 0.0;
            for (int i = k; i < 5; ++i) d += v[i] * A[i][j];
            d *= tau;
            for (int i = k; i < 5; ++i) A[i][j] -= d * v[i];
        }
        { double d = 0.0; for (int i = k; i < 5; ++i) d += v[i] * b[i]; d *= tau; for (int i = k; i < 5; ++i) b[i] -= d * v[i]; }
        A[k][k] = beta;
        for (int i = k + 1; i < 5; ++i) A[i][k] = 0.0;
    }
    double z[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        if (i >= rank) continue;
        double sacc = b[i];
        for (int j = i + 1; j < 3; ++j) if (j < rank) sacc -= A[i][j] * z[j];
        z[i] = sacc / A[i][i];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) if (perm[k] == c) x[c] = z[k];
}

/* pointAssociateToMap (:125-134) of stack point po */
__device__ __forceinline__ void ll_map_to_world(const double *pose, const float4 po, float &sx, float &sy, float &sz)
{
    const double ux = pose[0], uy = pose[1], uz = pose[2], w = pose[3];
    const double v[3] = {(double)po.x, (double)po.y, (double)po.z};
    double uvx = uy * v[2] - uz * v[1], uvy = uz * v[0] - ux * v[2], uvz = ux * v[1] - uy * v[0];
    uvx += uvx; uvy += uvy; uvz += uvz;
    sx = (float)(((v[0] + w * uvx) + (uy * uvz - uz * uvy)) + pose[4]);
    sy = (float)(((v[1] + w * uvy) + (uz * uvx - ux * uvz)) + pose[5]);
    sz = (float)(((v[2] + w * uvz) + (ux * uvy - uy * uvx)) + pose[6]);
}

/* R(q)^-1 (s - t): the conjugate quaternion through ll_map_to_world's operations in their order, the pose used as given
 * (ll_visibility's vote and ll_bev's prepare take a world point into a frame with it) */
__device__ __forceinline__ void vis_world_to_frame(const double *pose, float sx, float sy, float sz, float &lx, float &ly, float &lz)
{
    const double ux = -pose[0], uy = -pose[1], uz = -pose[2], w = pose[3];
    const double v[3] = {(double)sx - pose[4], (double)sy - pose[5], (double)sz - pose[6]};
    double uvx = uy * v[2] - uz * v[1], uvy = uz * v[0] - ux * v[2], uvz = ux * v[1] - uy * v[0];
    uvx += uvx; uvy += uvy; uvz += uvz;
    lx = (float)((v[0] + w * uvx) + (uy * uvz - uz * uvy));
    ly = (float)((v[1] + w * uvy) + (uz * uvx - ux * uvz));
    lz = (float)((v[2] + w * uvz) + (ux * uvy - uy * uvx));
}

/* residual block `pos` of cloud type `which` <- the fit of stack point i (ll_map_fit leaves it in q*, the solves read f*) */
__device__ __forceinline__ void ll_map_place(const LLMapView &M, int which, int pos, int i)
{
    M.src[which][pos] = i;
    if (which == 0) for (int k = 0; k < 3; ++k) { M.fa[(size_t)pos * 3 + k] = M.qa[(size_t)i * 3 + k]; M.fb[(size_t)pos * 3 + k] = M.qb[(size_t)i * 3 + k]; }
    else { for (int k = 0; k < 3; ++k) M.fn[(size_t)pos * 3 + k] = M.qn[(size_t)i * 3 + k]; M.fd[pos] = M.qd[i]; }
}

/* insertion of (d, j[, p]) into five slots kept ascending by (distance, index) */
template <bool WITH_PT>
__device__ __forceinline__ void ll_five_insert(float bd[5], int bi[5], float4 bp[5], int &nb, float d, int j, const float4 &p)
{
    if (d < bd[4] || (d == bd[4] && j < bi[4])) {
        bd[4] = d; bi[4] = j;
        if (WITH_PT) bp[4] = p;
#pragma unroll
        for (int s = 4; s > 0; --s)
            if (bd[s] < bd[s - 1] || (bd[s] == bd[s - 1] && bi[s] < bi[s - 1])) {
                const float td = bd[s]; bd[s] = bd[s - 1]; bd[s - 1] = td;
                const int ti = bi[s]; bi[s] = bi[s - 1]; bi[s - 1] = ti;
                if (WITH_PT) { const float4 tp = bp[s]; bp[s] = bp[s - 1]; bp[s - 1] = tp; }
            }
        if (nb < 5) ++nb;
    }
}

/* exact K = 5 over the 27 cells around the query, ascending (distance, index).  gid == nullptr: index = position in the
 * search cloud; otherwise the caller's global id of the point (a tile shard of a larger cloud, same tie order). */
template <bool WITH_PT>
__device__ __forceinline__ void ll_map_search5(const LLGrid3 &G, int n_map, const int *gid, float sx, float sy, float sz,
                                               float bd[5], int bi[5], float4 bp[5], int &nb)
{
    nb = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) { bd[k] = INFINITY; bi[k] = INT_MAX; if (WITH_PT) bp[k] = make_float4(0.f, 0.f, 0.f, 0.f); }
    if (n_map <= 0) return;
    int cx = (int)floorf((sx - G.org[0]) / G.cell), cy = (int)floorf((sy - G.org[1]) / G.cell), cz = (int)floorf((sz - G.org[2]) / G.cell);
    cx = min(max(cx, 0), G.dim[0] - 1); cy = min(max(cy, 0), G.dim[1] - 1); cz = min(max(cz, 0), G.dim[2] - 1);
    /* the nine (z, y) rows of the 27 cells: the three x-cells of a row are contiguous, so a row is one range.  All eighteen
     * bounds first (independent loads): a thread's search is a chain of dependent round trips, and a frame's association is
     * ~11 k of them on a chip that holds 65 k threads. */
    int st[9], en[9];
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, G.dim[0] - 1);
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int yy = cy + (r % 3) - 1, zz = cz + (r / 3) - 1;
        st[r] = 0; en[r] = 0;
        if (yy >= 0 && zz >= 0 && yy < G.dim[1] && zz < G.dim[2]) {
            const int row = (zz * G.dim[1] + yy) * G.dim[0];
            st[r] = G.start[row + x0]; en[r] = G.start[row + x1 + 1];
        }
    }
    /* all nine ranges advance together, two points of each per round: the five best are a total order on (distance, index), so
     * the order of insertion does not matter, and a search is 2-3 round trips of up to eighteen loads instead of nine chains */
    for (;;) {
        float4 p[9][2];
        bool any = false;
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
            for (int u = 0; u < 2; ++u) if (st[r] + u < en[r]) { p[r][u] = G.pts[st[r] + u]; any = true; }
        if (!any) break;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (st[r] + u >= en[r]) continue;
                float diff = sx - p[r][u].x; float d = diff * diff;            /* FLANN L2_Simple: a = query, b = data */
                diff = sy - p[r][u].y; d += diff * diff;
                diff = sz - p[r][u].z; d += diff * diff;
                int j = __float_as_int(p[r][u].w);
                if (WITH_PT && gid) j = gid[j];
                ll_five_insert<WITH_PT>(bd, bi, bp, nb, d, j, p[r][u]);
            }
            st[r] += 2;
        }
    }
}

/* the five neighbours of stack point i -> line (eigen test, :1888-1930) or plane (QR fit, :1960-2000) */
template <bool CORNER>
__device__ __forceinline__ void ll_map_fit(const LLMapView &M, int i, const double P5[5][3])
{
    const int which = CORNER ? 0 : 1;
    unsigned char ok = 0;
    if (CORNER) {
        double c[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 5; ++j) for (int k = 0; k < 3; ++k) c[k] = c[k] + P5[j][k];              /* :1888-1895 */
        for (int k = 0; k < 3; ++k) c[k] = c[k] / 5.0;
        double cov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
        for (int j = 0; j < 5; ++j) {                                                                  /* :1898-1903 */
            const double z[3] = {P5[j][0] - c[0], P5[j][1] - c[1], P5[j][2] - c[2]};
            for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) cov[a][b] = cov[a][b] + z[a] * z[b];
        }
        double w[3], V[3][3];
        ll_sym_eig3(cov, w, V);
        if (w[2] > 3 * w[1]) {                                                                         /* :1911 */
            ok = 1;
            for (int k = 0; k < 3; ++k) { M.qa[(size_t)i * 3 + k] = 0.1 * V[k][2] + c[k]; M.qb[(size_t)i * 3 + k] = -0.1 * V[k][2] + c[k]; }
        }
    } else {
        double A[5][3], b[5] = {-1.0, -1.0, -1.0, -1.0, -1.0}, nrm[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 5; ++j) for (int k = 0; k < 3; ++k) A[j][k] = P5[j][k];
        ll_qr_solve_5x3(A, b, nrm);                                                                     /* :1972 */
        const double len = sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
        const double nd = 1 / len;                                                                     /* :1973 */
        if (len * len > 0.0) { nrm[0] /= len; nrm[1] /= len; nrm[2] /= len; }                        /* :1974 */
        bool valid = true;
#pragma unroll
        for (int j = 0; j < 5; ++j)                                                                    /* :1980-1990 */
            if (fabs(nrm[0] * P5[j][0] + nrm[1] * P5[j][1] + nrm[2] * P5[j][2] + nd) > 0.2) valid = false;
        if (valid) {
            ok = 1;
            for (int k = 0; k < 3; ++k) M.qn[(size_t)i * 3 + k] = nrm[k];
            M.qd[i] = nd;
            if (M.ctr) {                                                                               /* the vote's Corre_Match.tgt (:1949, :1960-1962, :1969-1971) */
                float c[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < 5; ++j) for (int k = 0; k < 3; ++k) c[k] += (float)P5[j][k];      /* P5 holds floats: the conversion back is exact */
                for (int k = 0; k < 3; ++k) M.ctr[(size_t)i * 3 + k] = c[k] / 5.0f;
            }
        }
    }
    M.ok[which][i] = ok;
}

#define LL_KNNB 64            /* threads per workgroup of the searches: ~11 k stack points should spread over the chip, not fill 45 workgroups */
template <bool CORNER>
__device__ __forceinline__ void ll_map_knn_one(const LLMapView &M, int i)
{
    const int which = CORNER ? 0 : 1;
    if (i >= M.n_stk[which]) return;
    float sx, sy, sz;
    ll_map_to_world(M.pose, M.stk[which][i], sx, sy, sz);
    float bd[5]; int bi[5]; int nb; float4 unused[1];
    ll_map_search5<false>(M.grid[which], M.n_map[which], nullptr, sx, sy, sz, bd, bi, unused, nb);
    if (nb == 5 && bd[4] < 1.0f) {                                                                     /* :1885, :1958 */
        const float4 *cloud = M.map[which];
        double P5[5][3];
#pragma unroll
        for (int j = 0; j < 5; ++j) { const float4 p = cloud[bi[j]]; P5[j][0] = p.x; P5[j][1] = p.y; P5[j][2] = p.z; }
        ll_map_fit<CORNER>(M, i, P5);
    } else M.ok[which][i] = 0;
}
