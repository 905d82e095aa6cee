/*
 * ll_posegraph.hip -- ll_posegraphs: many independent SE(3) pose graphs optimised side by side, one workgroup per graph, the whole
 * Levenberg-Marquardt solve in ONE launch.  Not in the reference; the contract is in include/lightloam_hip.h.
 *
 * The problem.  Poses P_k = (q_k, t_k), world from body, pose_w7 layout.  Edge e = (i, j, Z, s, a) measures Z ~ P_i^-1 P_j:
 *     q_e = q_z* (x) q_i* (x) q_j,   t_e = R(q_z)^T (R(q_i)^T (t_j - t_i) - t_z),   r = s o [2 sgn(w_e) vec(q_e) ; t_e],  sgn(0) = +1,
 *     cost = 1/2 sum_e rho_a(|r_e|^2), rho_a = ceres::HuberLoss(a) (a <= 0: none).
 * The increment of a node is d = (w, dt), six numbers, applied by ll_pose_plus: q <- exp(w) (x) q with exp(w) = [sin|w| w/|w|, cos|w|]
 * (w is the HALF-angle vector, the rotation it stands for is R(exp w) = I + 2 [w]x + O(w^2)), t <- t + dt.
 *
 * Jacobians (f64, closed form, at d = 0).  Write a = q_z* (x) q_i*, so that q_e = a (x) q_j and R(a) = R(q_z)^T R(q_i)^T, and v = t_j - t_i.
 *   node j, rotation:  q_j <- [w, 1] (x) q_j  gives  q_e + a (x) [w, 0] (x) q_j, which is linear in w:
 *                      d r_rot / d w_j = A,  column k of A = 2 sgn(w_e) vec(a (x) e_k (x) q_j),  e_k the pure unit quaternion of axis k.
 *   node i, rotation:  q_i* <- q_i* (x) [-w, 1]  gives  q_e - a (x) [w, 0] (x) q_j:  d r_rot / d w_i = -A.
 *                      R(q_i)^T <- R(q_i)^T (I - 2 [w]x):  t_e changes by -2 R(a) (w x v) = 2 R(a) [v]x w:  d t_e / d w_i = 2 R(a) [v]x.
 *   translations:      d t_e / d t_j = R(a),  d t_e / d t_i = -R(a);  t_e does not depend on w_j, r_rot on no translation.
 *       J_i = S [ -A  0 ; 2 R(a)[v]x  -R(a) ],   J_j = S [ A  0 ; 0  R(a) ],   S = diag(s).
 * An ll_pg_edge6 carries a full 6 x 6 matrix S in place of diag(s): r = S e and J = S J^e with e and J^e the unweighted error and
 * Jacobians above (pg_error yields them for both edge types).  Everything from the Huber scale on is one text, the kernel a template
 * over the edge type; the diagonal calls keep their own instantiation.
 * The Gauss-Newton model takes r and J times sqrt(rho') (ll_huber_scale: Ceres' corrector where rho'' <= 0), so g = J^T r is the
 * gradient of the robust cost.
 *
 * k_pg_solve, graph = blockIdx.x, 256 threads, the per-graph workspace in HBM (at KITTI-00 size a few MB, L2-resident), LDS only for
 * the reductions.  No grid barrier, no spin, no floating-point atomic; every loop is bounded by an option.  Per LM iteration:
 *   linearise   a thread per edge: r, J_i, J_j, the Huber scale, then H_ij = J_i^T J_j, H_ii, H_jj (36 doubles each) and the two gradient
 *               parts into the edge's own slots.  A thread per node then sums its diagonal block and gradient over its incident edges
 *               in edge order (the CSR list the host built) -- a fixed order, so the bits do not depend on scheduling.
 *   solve       (H + D / radius) d = -g by preconditioned conjugate gradients, D = the clamped diagonal of H as in ll_lm_step.h, the
 *               preconditioner block-Jacobi: ll_chol_solve on every node's damped 6 x 6 block.  A thread per node does the mat-vec
 *               over its incident edges' H_ij.  Dot products: thread-strided partial sums, then a fixed tree over the 256 partials (pg_sum2).
 *               Stops at |r| <= eta |g|, at max_pcg_iterations, or at a p^T A p that is not positive and finite (the iterate so far
 *               stays: CG's energy decreases monotonically, so it is the best one).  With ll_posegraphs_set_preconditioner(CHAIN) the
 *               second instantiation of the kernel preconditions with the block-tridiagonal part of the matrix instead, by block
 *               cyclic reduction inside the workgroup (further down); the block-Jacobi instantiation is the text as it was.
 *   accept      ll_lm_step.h's policy over all nodes: model cost change -(g.d + d.H d / 2), the parameter and function tests, rho, the
 *               radius update by 1 - (2 rho - 1)^3, a decrease factor that doubles with every rejection.  The candidate is judged by a
 *               cost-only pass over the edges; an accepted one is linearised anew.
 * Every index is relative to the graph and every sum has a fixed shape, so a graph's poses and record have the same bits alone, in any
 * batch and at any position.  A non-finite cost, gradient or step ends the graph's solve with termination 5 and the last accepted poses.
 */
#include "ll_internal.h"
#include "ll_factor_math.h"
#include <algorithm>
#include <cmath>
#include <numeric>

#define PG_THREADS 256
#define PG_NODE_DOUBLES 92                    /* x 7, cand 7, Hd 36, g 6, D 6, d 6, r 6, z 6, p 6, Ap 6 */
#define PG_EDGE_DOUBLES 121                   /* H_ij, H_ii, H_jj 36 each, g_i, g_j 6 each, cost */

template <typename Edge>                      /* ll_pg_edge: diagonal square-root information; ll_pg_edge6: a full 6 x 6 one */
struct PgArgs {
    /* the call's input, as the host packed it */
    const double *pose_in; const Edge *edges; const int *node_off, *edge_off, *inc_off, *inc, *inc_nb; const unsigned char *fixed;
    /* workspace, [nodes_total] or [edges_total] rows */
    double *x, *cand, *Hd, *g, *D, *d, *r, *z, *p, *Ap, *eH, *eg, *ecost;
    /* results: solve -> poses [nodes][7] + records; evaluate -> gradients [nodes][6] + costs */
    double *out_nodes; ll_pg_record *rec; double *out_cost;
    ll_pg_options o;
    int solve;
    /* the chain preconditioner's workspace, [nodes_total] rows, and its counts [graphs][2]; NULL under block-Jacobi */
    double *cD, *cWL, *cWR, *cC, *cr; int *cstat;
};

struct ll_posegraphs {
    ll_ctx *ctx = nullptr;
    int max_graphs = 0, max_nodes = 0, max_edges = 0;
    unsigned char *d_in = nullptr, *d_out = nullptr;
    double *d_ws = nullptr;
    size_t in_bytes = 0, out_bytes = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms[2] = {0.0, 0.0};
    long long counts[3] = {0, 0, 0};
    int precond = LL_PG_PRECOND_BLOCK_JACOBI;
    double *d_chain = nullptr;                 /* allocated when the chain preconditioner (or ll_posegraphs_chain_solve) is first asked for */
    long long pc_counts[2] = {0, 0};
    unsigned char *d_cov = nullptr;            /* the covariances' tables and columns: allocated at the first call, grown when a call needs more */
    size_t cov_bytes = 0;
    hipEvent_t cov_ev[3] = {nullptr, nullptr, nullptr};
    double cov_ms[2] = {0.0, 0.0};
    long long cov_counts[3] = {0, 0, 0};
    std::string err;
};

/* ------------------------------------------------------------------ one edge: the kernels' text and ll_pg_edge_gate's
 * the UNWEIGHTED error er = [2 sgn(w_e) vec(q_e) ; t_e] of an edge at the unit poses (Pi, Pj), with a = qzc (x) q_i*, q_e = a (x) q_j and
 * t_e = R(a) (t_j - t_i) - R(qzc) t_z; qzc is the unit conjugate of the measurement's quaternion, t_z its translation.  With A != NULL
 * also what the Jacobians are made of: A (3 x 3, see above), Ra = R(a), v = t_j - t_i.  R(a) v is the matrix form.  z_matrix_form says
 * which form R(qzc) t_z takes: the kernels have always used the Eigen form and ll_pg_edge_gate the matrix form, and the two round
 * differently, so each caller keeps its bits */
LL_HD void pg_error(const double *Pi, const double *Pj, const double *qzc, const double *t_z, bool z_matrix_form, double er[6], double (*A)[3], double (*Ra)[3], double *v)
{
    const double qic[4] = {-Pi[0], -Pi[1], -Pi[2], Pi[3]};
    double a[4], qe[4], R[3][3], te[3], tz[3];
    ll_qmul(qzc, qic, a);
    ll_qmul(a, Pj, qe);
    const double sgn = qe[3] < 0.0 ? -1.0 : 1.0;
    ll_quat_matrix(a, R);
    const double dv[3] = {Pj[4] - Pi[4], Pj[5] - Pi[5], Pj[6] - Pi[6]};
    if (z_matrix_form) { double Rz[3][3]; ll_quat_matrix(qzc, Rz); ll_mat_apply(Rz, t_z, tz); }
    else ll_rotate(qzc, t_z, tz);
    for (int k = 0; k < 3; ++k) te[k] = (R[k][0] * dv[0] + R[k][1] * dv[1]) + R[k][2] * dv[2];   /* ll_mat_apply's row, kept in place (below) */
    for (int k = 0; k < 3; ++k) {
        er[k] = 2.0 * sgn * qe[k];
        er[3 + k] = te[k] - tz[k];
    }
    if (!A) return;
    for (int k = 0; k < 3; ++k) {
        double ek[4] = {0.0, 0.0, 0.0, 0.0}, ae[4], c[4];
        ek[k] = 1.0;
        ll_qmul(a, ek, ae);
        ll_qmul(ae, Pj, c);
        for (int m = 0; m < 3; ++m) { A[m][k] = 2.0 * sgn * c[m]; Ra[m][k] = R[m][k]; }
        v[k] = dv[k];
    }
}

/* the unweighted Jacobians Je_i = [ -A  0 ; 2 R(a)[v]x  -R(a) ], Je_j = [ A  0 ; 0  R(a) ], for ll_pg_edge_gate.  The kernels keep
 * three lines of this file's arithmetic in place -- this assembly in both pg_edge_linearise, the row of R(a) v in pg_error, the
 * normalisation on entry: with the shared functions there the device code differs from its predecessor's (at least in the operand
 * order of some v_mul_f64) and measured outside that code's own run-to-run band in some configurations */
LL_HD void pg_jacobians(const double (*A)[3], const double (*Ra)[3], const double *v, double (*Jei)[6], double (*Jej)[6])
{
    const double vx[3][3] = {{0.0, -v[2], v[1]}, {v[2], 0.0, -v[0]}, {-v[1], v[0], 0.0}};
    for (int m = 0; m < 3; ++m)
        for (int k = 0; k < 3; ++k) {
            Jei[m][k] = -A[m][k];            Jei[m][3 + k] = 0.0;
            Jej[m][k] = A[m][k];             Jej[m][3 + k] = 0.0;
            Jei[3 + m][k] = 2.0 * ((Ra[m][0] * vx[0][k] + Ra[m][1] * vx[1][k]) + Ra[m][2] * vx[2][k]);
            Jei[3 + m][3 + k] = -Ra[m][k];
            Jej[3 + m][k] = 0.0;             Jej[3 + m][3 + k] = Ra[m][k];
        }
}

/* ------------------------------------------------------------------ device: one edge
 * pg_error of an edge as the graph stores it: Z normalised here, R(q_z)^T t_z in the Eigen form */
__device__ __forceinline__ void pg_error_z(const double *Pi, const double *Pj, const double *Z_w7, double er[6], double (*A)[3], double (*Ra)[3], double *v)
{
    const double zc[4] = {-Z_w7[0], -Z_w7[1], -Z_w7[2], Z_w7[3]};
    double qzc[4];
    ll_quat_unit(zc, qzc);
    pg_error(Pi, Pj, qzc, Z_w7 + 4, false, er, A, Ra, v);
}

/* the weighted residual r = S er: diag(sqrt_info), or the full matrix row by row, columns ascending */
__device__ __forceinline__ void pg_residual(const double *Pi, const double *Pj, const ll_pg_edge &e, double r[6], double (*A)[3], double (*Ra)[3], double *v)
{
    double er[6];
    pg_error_z(Pi, Pj, e.Z_w7, er, A, Ra, v);
    for (int k = 0; k < 6; ++k) r[k] = e.sqrt_info[k] * er[k];
}
__device__ __forceinline__ void pg_residual(const double *Pi, const double *Pj, const ll_pg_edge6 &e, double r[6], double (*A)[3], double (*Ra)[3], double *v)
{
    double er[6];
    pg_error_z(Pi, Pj, e.Z_w7, er, A, Ra, v);
    for (int m = 0; m < 6; ++m) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += e.S[m * 6 + k] * er[k];
        r[m] = s;
    }
}

template <typename Edge>
__device__ __forceinline__ double pg_edge_cost(const double *Pi, const double *Pj, const Edge &e)
{
    double r[6], c = 0.0;
    pg_residual(Pi, Pj, e, r, nullptr, nullptr, nullptr);
    const double sq = ((r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3])) + (r[4] * r[4] + r[5] * r[5]);
    (void)ll_huber_scale(sq, e.huber, c);
    return c;
}

/* the edge's slots: eH[0] = J_i^T J_j, eH[1] = J_i^T J_i, eH[2] = J_j^T J_j, eg[0] = J_i^T r, eg[1] = J_j^T r, and its cost */
__device__ __forceinline__ void pg_edge_products(const double (*Ji)[6], const double (*Jj)[6], const double *r, double *eH, double *eg)
{
    for (int a = 0; a < 6; ++a) {
        double gi = 0.0, gj = 0.0;
        for (int m = 0; m < 6; ++m) { gi += Ji[m][a] * r[m]; gj += Jj[m][a] * r[m]; }
        eg[a] = gi; eg[6 + a] = gj;
        for (int b = 0; b < 6; ++b) {
            double hij = 0.0, hii = 0.0, hjj = 0.0;
            for (int m = 0; m < 6; ++m) { hij += Ji[m][a] * Jj[m][b]; hii += Ji[m][a] * Ji[m][b]; hjj += Jj[m][a] * Jj[m][b]; }
            eH[a * 6 + b] = hij; eH[36 + a * 6 + b] = hii; eH[72 + a * 6 + b] = hjj;
        }
    }
}

__device__ __forceinline__ void pg_edge_linearise(const double *Pi, const double *Pj, const ll_pg_edge &e, double *eH, double *eg, double *ecost)
{
    double r[6], A[3][3], Ra[3][3], v[3], Ji[6][6], Jj[6][6], c = 0.0;
    pg_residual(Pi, Pj, e, r, A, Ra, v);
    const double sq = ((r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3])) + (r[4] * r[4] + r[5] * r[5]);
    const double w = ll_huber_scale(sq, e.huber, c);
    *ecost = c;
    const double vx[3][3] = {{0.0, -v[2], v[1]}, {v[2], 0.0, -v[0]}, {-v[1], v[0], 0.0}};
    for (int m = 0; m < 3; ++m) {
        const double sr = w * e.sqrt_info[m], st = w * e.sqrt_info[3 + m];
        for (int k = 0; k < 3; ++k) {
            Ji[m][k] = -sr * A[m][k];        Ji[m][3 + k] = 0.0;
            Jj[m][k] = sr * A[m][k];         Jj[m][3 + k] = 0.0;
            Ji[3 + m][k] = st * (2.0 * ((Ra[m][0] * vx[0][k] + Ra[m][1] * vx[1][k]) + Ra[m][2] * vx[2][k]));
            Ji[3 + m][3 + k] = -st * Ra[m][k];
            Jj[3 + m][k] = 0.0;              Jj[3 + m][3 + k] = st * Ra[m][k];
        }
    }
    for (int m = 0; m < 6; ++m) r[m] *= w;
    pg_edge_products(Ji, Jj, r, eH, eg);
}

/* the full variant: the unweighted Jacobians Je_i, Je_j as pg_jacobians states them, then J = w S Je */
__device__ __forceinline__ void pg_edge_linearise(const double *Pi, const double *Pj, const ll_pg_edge6 &e, double *eH, double *eg, double *ecost)
{
    double r[6], A[3][3], Ra[3][3], v[3], Jei[6][6], Jej[6][6], Ji[6][6], Jj[6][6], c = 0.0;
    pg_residual(Pi, Pj, e, r, A, Ra, v);
    const double sq = ((r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3])) + (r[4] * r[4] + r[5] * r[5]);
    const double w = ll_huber_scale(sq, e.huber, c);
    *ecost = c;
    const double vx[3][3] = {{0.0, -v[2], v[1]}, {v[2], 0.0, -v[0]}, {-v[1], v[0], 0.0}};
    for (int m = 0; m < 3; ++m)
        for (int k = 0; k < 3; ++k) {
            Jei[m][k] = -A[m][k];            Jei[m][3 + k] = 0.0;
            Jej[m][k] = A[m][k];             Jej[m][3 + k] = 0.0;
            Jei[3 + m][k] = 2.0 * ((Ra[m][0] * vx[0][k] + Ra[m][1] * vx[1][k]) + Ra[m][2] * vx[2][k]);
            Jei[3 + m][3 + k] = -Ra[m][k];
            Jej[3 + m][k] = 0.0;             Jej[3 + m][3 + k] = Ra[m][k];
        }
    for (int m = 0; m < 6; ++m)
        for (int k = 0; k < 6; ++k) {
            double si = 0.0, sj = 0.0;
            for (int n = 0; n < 6; ++n) { si += e.S[m * 6 + n] * Jei[n][k]; sj += e.S[m * 6 + n] * Jej[n][k]; }
            Ji[m][k] = w * si; Jj[m][k] = w * sj;
        }
    for (int m = 0; m < 6; ++m) r[m] *= w;
    pg_edge_products(Ji, Jj, r, eH, eg);
}

/* ------------------------------------------------------------------ device: the workgroup's sums
 * A fixed tree over the 256 partials: an xor butterfly inside each wave (a + b == b + a bit for bit, so all 64 lanes end with the same
 * value), then the four waves' sums as (w0 + w1) + (w2 + w3) by every thread.  sh: 8 doubles. */
__device__ __forceinline__ void pg_sum2(double &a, double &b, double *sh)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[wave] = a; sh[4 + wave] = b; }
    __syncthreads();
    a = (sh[0] + sh[1]) + (sh[2] + sh[3]); b = (sh[4] + sh[5]) + (sh[6] + sh[7]);
    __syncthreads();
}

__device__ __forceinline__ double pg_max2(double u, double w) { return (u != u || w != w) ? __builtin_nan("") : (u > w ? u : w); }   /* fmax would drop a NaN */

__device__ __forceinline__ double pg_max(double a, double *sh)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a = pg_max2(a, __shfl_xor(a, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    const double m = pg_max2(pg_max2(sh[0], sh[1]), pg_max2(sh[2], sh[3]));
    __syncthreads();
    return m;
}

/* ------------------------------------------------------------------ device: one graph */
template <typename Edge>
struct PgGraph {                               /* the graph's rows of the workspace */
    int N, E, n0, e0;
    const Edge *edges; const int *inc_off, *inc, *inc_nb; const unsigned char *fixed;
    double *x, *cand, *Hd, *g, *D, *d, *r, *z, *p, *Ap, *eH, *eg, *ecost;
};

/* edges at the poses `P`, then the nodes' sums; -> the cost (every thread) */
template <typename Edge>
__device__ double pg_linearise(const PgGraph<Edge> &G, const double *P, const ll_pg_options &o, double *sh)
{
    const int tid = threadIdx.x;
    double c = 0.0, unused = 0.0;
    for (int e = tid; e < G.E; e += PG_THREADS) {
        const Edge &ed = G.edges[e];
        pg_edge_linearise(P + (size_t)ed.i * 7, P + (size_t)ed.j * 7, ed, G.eH + (size_t)e * 108, G.eg + (size_t)e * 12, G.ecost + e);
        c += G.ecost[e];
    }
    pg_sum2(c, unused, sh);                                        /* its barriers also publish the edges' slots */
    for (int n = tid; n < G.N; n += PG_THREADS) {
        double H[36], g[6];
        for (int k = 0; k < 36; ++k) H[k] = 0.0;
        for (int k = 0; k < 6; ++k) g[k] = 0.0;
        for (int q = G.inc_off[G.n0 + n]; q < G.inc_off[G.n0 + n + 1]; ++q) {      /* ascending edges */
            const int code = G.inc[q], e = code >> 1, side = code & 1;
            const double *eH = G.eH + (size_t)e * 108 + 36 + 36 * side, *eg = G.eg + (size_t)e * 12 + 6 * side;
            for (int k = 0; k < 36; ++k) H[k] += eH[k];
            for (int k = 0; k < 6; ++k) g[k] += eg[k];
        }
        const bool fx = G.fixed[n] != 0;
        for (int k = 0; k < 36; ++k) G.Hd[(size_t)n * 36 + k] = H[k];
        for (int k = 0; k < 6; ++k) {
            G.g[(size_t)n * 6 + k] = fx ? 0.0 : g[k];
            G.D[(size_t)n * 6 + k] = fmin(fmax(H[k * 6 + k], o.min_lm_diagonal), o.max_lm_diagonal);
        }
    }
    __syncthreads();
    return c;
}

/* out = (H + damp D) in, rows of fixed nodes 0 (their `in` is 0 as well); a thread per node */
template <typename Edge>
__device__ void pg_matvec(const PgGraph<Edge> &G, const double *in, double *out, double damp)
{
    for (int n = threadIdx.x; n < G.N; n += PG_THREADS) {
        double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (!G.fixed[n]) {
            const double *H = G.Hd + (size_t)n * 36, *u = in + (size_t)n * 6;
            for (int a = 0; a < 6; ++a) {
                double s = damp * G.D[(size_t)n * 6 + a] * u[a];
                for (int b = 0; b < 6; ++b) s += H[a * 6 + b] * u[b];
                y[a] = s;
            }
            for (int q = G.inc_off[G.n0 + n]; q < G.inc_off[G.n0 + n + 1]; ++q) {
                const int code = G.inc[q], e = code >> 1, side = code & 1;
                const double *Hij = G.eH + (size_t)e * 108, *w = in + (size_t)G.inc_nb[q] * 6;
                if (side == 0) { for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) y[a] += Hij[a * 6 + b] * w[b]; }
                else           { for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) y[a] += Hij[b * 6 + a] * w[b]; }
            }
        }
        for (int a = 0; a < 6; ++a) out[(size_t)n * 6 + a] = y[a];
    }
}

/* z = M^-1 r of node n, M = Hd + D / radius; false where M is not positive definite (z = 0 then) */
template <typename Edge>
__device__ __forceinline__ bool pg_precondition(const PgGraph<Edge> &G, int n, double inv_radius, const double r[6], double z[6])
{
    double M[36], nr[6];
    for (int k = 0; k < 36; ++k) M[k] = G.Hd[(size_t)n * 36 + k];
    for (int k = 0; k < 6; ++k) { M[k * 6 + k] += G.D[(size_t)n * 6 + k] * inv_radius; nr[k] = -r[k]; }
    if (ll_chol_solve(M, nr, z) != 0) { for (int k = 0; k < 6; ++k) z[k] = 0.0; return false; }
    return true;
}

__device__ __forceinline__ bool pg_finite(double v) { return v - v == 0.0; }

/* ------------------------------------------------------------------ device: the chain preconditioner
 * M = the block-tridiagonal part of H + D / radius in node order (the contract is in the header), solved by block cyclic reduction
 * inside the workgroup.  Level l, stride s = 2^l: the nodes n = s, 3s, 5s, ... are eliminated -- D_n is factored in place (Cholesky,
 * lower triangle, the reciprocals of L's diagonal on the diagonal), W_left = M[n-s][n] D_n^-1 and W_right = M[n+s][n] D_n^-1 are formed
 * a row at a time --, then every survivor a = 0, 2s, 4s, ... takes D_a -= W M[n][a] from its left eliminated neighbour, then from its
 * right one, and the coupling to the next survivor, M[a][a+2s] = -W_left(a+s) M[a+s][a+2s].  C[a] is M[a][a + s] of the level at hand.
 * Everything is relative to the system and every sum has a fixed shape; a thread holds one triangular factor and one row at a time. */
struct PgChain { int N; double *D, *WL, *WR, *C, *r; };           /* one system's rows of the workspace */

/* the lower triangle of A (row-major 6 x 6, in memory) -> L with L L^T = A, kept in registers as L[i * 6 + j], j < i, and 1 / L_ii on
 * the diagonal; false at a pivot that is not positive and finite (L is not to be used then) */
__device__ __forceinline__ bool pg_chol6(const double *A, double L[36])
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double acc = A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) acc -= L[i * 6 + k] * L[j * 6 + k];
            if (i == j) { ok = ok && acc > 0.0 && pg_finite(acc); L[i * 6 + i] = 1.0 / sqrt(acc); }
            else L[i * 6 + j] = acc * L[j * 6 + j];
        }
    return ok;
}

__device__ __forceinline__ void pg_chol6_store(const double L[36], double *A)
{
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) A[i * 6 + j] = L[i * 6 + j];
}

__device__ __forceinline__ void pg_chol6_load(const double *A, double L[36])
{
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) L[i * 6 + j] = A[i * 6 + j];
}

/* v <- (L L^T)^-1 v */
__device__ __forceinline__ void pg_chol6_solve(const double L[36], double v[6])
{
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double acc = v[i];
#pragma unroll
        for (int k = 0; k < i; ++k) acc -= L[i * 6 + k] * v[k];
        v[i] = acc * L[i * 6 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double acc = v[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) acc -= L[k * 6 + i] * v[k];
        v[i] = acc * L[i * 6 + i];
    }
}

/* y -= W x (t == 0) or y -= W^T x (t == 1), W row-major in memory */
__device__ __forceinline__ void pg_sub_matvec6(const double *W, const double *x, double y[6], int t)
{
    double u[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) u[k] = x[k];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double acc = y[a];
#pragma unroll
        for (int b = 0; b < 6; ++b) acc -= (t ? W[b * 6 + a] : W[a * 6 + b]) * u[b];
        y[a] = acc;
    }
}

/* Factorises the system whose diagonal blocks are in S.D and couplings M[n][n+1] in S.C (the last one is not read); both are overwritten.
 * -> true, the same in every thread, iff every pivot was positive and finite.  Ends behind a barrier. */
__device__ bool pg_chain_factor(const PgChain &S, double *sh)
{
    const long long N = S.N;
    double bad = 0.0;
    for (long long s = 1; s < N; s <<= 1) {
        for (long long n = s + 2 * s * threadIdx.x; n < N; n += 2 * s * PG_THREADS) {           /* eliminate */
            double L[36], v[6];
            double *Dn = S.D + (size_t)n * 36;
            if (!pg_chol6(Dn, L)) bad = 1.0;
            pg_chol6_store(L, Dn);
            const double *Ca = S.C + (size_t)(n - s) * 36, *Cn = S.C + (size_t)n * 36;
            double *WL = S.WL + (size_t)n * 36, *WR = S.WR + (size_t)n * 36;
#pragma unroll 1
            for (int i = 0; i < 6; ++i) {                          /* row i of M[n-s][n] D_n^-1 = (D_n^-1 row_i(M[n-s][n])^T)^T */
#pragma unroll
                for (int k = 0; k < 6; ++k) v[k] = Ca[i * 6 + k];
                pg_chol6_solve(L, v);
#pragma unroll
                for (int k = 0; k < 6; ++k) WL[i * 6 + k] = v[k];
            }
            if (n + s < N) {
#pragma unroll 1
                for (int i = 0; i < 6; ++i) {                      /* M[n+s][n] = M[n][n+s]^T: its row i is column i of C[n] */
#pragma unroll
                    for (int k = 0; k < 6; ++k) v[k] = Cn[k * 6 + i];
                    pg_chol6_solve(L, v);
#pragma unroll
                    for (int k = 0; k < 6; ++k) WR[i * 6 + k] = v[k];
                }
            }
        }
        __syncthreads();
        for (long long a = 2 * s * threadIdx.x; a < N; a += 2 * s * PG_THREADS) {               /* gather: left neighbour, then right */
            double *Da = S.D + (size_t)a * 36, *Ca = S.C + (size_t)a * 36;
            if (a >= s) {
                const double *W = S.WR + (size_t)(a - s) * 36, *Cl = S.C + (size_t)(a - s) * 36;           /* M[a][l] D_l^-1, M[l][a] */
#pragma unroll 1
                for (int i = 0; i < 6; ++i) {
                    double w[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) w[k] = W[i * 6 + k];
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        double acc = Da[i * 6 + j];
#pragma unroll
                        for (int k = 0; k < 6; ++k) acc -= w[k] * Cl[k * 6 + j];
                        Da[i * 6 + j] = acc;
                    }
                }
            }
            if (a + s < N) {
                const double *W = S.WL + (size_t)(a + s) * 36, *Cr = S.C + (size_t)(a + s) * 36;           /* M[a][rt] D_rt^-1, M[rt][a+2s] */
#pragma unroll 1
                for (int i = 0; i < 6; ++i) {
                    double w[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) w[k] = W[i * 6 + k];
#pragma unroll
                    for (int j = 0; j < 6; ++j) {                  /* M[rt][a] = C[a]^T */
                        double acc = Da[i * 6 + j];
#pragma unroll
                        for (int k = 0; k < 6; ++k) acc -= w[k] * Ca[j * 6 + k];
                        Da[i * 6 + j] = acc;
                    }
                }
                if (a + 2 * s < N) {
#pragma unroll 1
                    for (int i = 0; i < 6; ++i) {                  /* C[a] is read no more: the next level's coupling goes there */
                        double w[6];
#pragma unroll
                        for (int k = 0; k < 6; ++k) w[k] = W[i * 6 + k];
#pragma unroll
                        for (int j = 0; j < 6; ++j) {
                            double acc = 0.0;
#pragma unroll
                            for (int k = 0; k < 6; ++k) acc -= w[k] * Cr[k * 6 + j];
                            Ca[i * 6 + j] = acc;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double L[36];
        if (!pg_chol6(S.D, L)) bad = 1.0;
        pg_chol6_store(L, S.D);
    }
    return !(pg_max(bad, sh) > 0.0);                              /* its barriers publish node 0's factor */
}

/* z = M^-1 r by the factors pg_chain_factor left: S.r holds r on entry (published) and is used up; z [N][6].  Ends behind a barrier. */
__device__ void pg_chain_apply(const PgChain &S, double *z)
{
    const long long N = S.N;
    long long top = 0;
    for (long long s = 1; s < N; s <<= 1) {
        top = s;
        for (long long a = 2 * s * threadIdx.x; a < N; a += 2 * s * PG_THREADS) {
            double y[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) y[k] = S.r[(size_t)a * 6 + k];
            if (a >= s) pg_sub_matvec6(S.WR + (size_t)(a - s) * 36, S.r + (size_t)(a - s) * 6, y, 0);
            if (a + s < N) pg_sub_matvec6(S.WL + (size_t)(a + s) * 36, S.r + (size_t)(a + s) * 6, y, 0);
#pragma unroll
            for (int k = 0; k < 6; ++k) S.r[(size_t)a * 6 + k] = y[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double L[36], y[6];
        pg_chol6_load(S.D, L);
#pragma unroll
        for (int k = 0; k < 6; ++k) y[k] = S.r[k];
        pg_chol6_solve(L, y);
#pragma unroll
        for (int k = 0; k < 6; ++k) z[k] = y[k];
    }
    __syncthreads();
    for (long long s = top; s >= 1; s >>= 1) {
        for (long long n = s + 2 * s * threadIdx.x; n < N; n += 2 * s * PG_THREADS) {
            double L[36], y[6];
            pg_chol6_load(S.D + (size_t)n * 36, L);
#pragma unroll
            for (int k = 0; k < 6; ++k) y[k] = S.r[(size_t)n * 6 + k];
            pg_chol6_solve(L, y);
            pg_sub_matvec6(S.WL + (size_t)n * 36, z + (size_t)(n - s) * 6, y, 1);
            if (n + s < N) pg_sub_matvec6(S.WR + (size_t)n * 36, z + (size_t)(n + s) * 6, y, 1);
#pragma unroll
            for (int k = 0; k < 6; ++k) z[(size_t)n * 6 + k] = y[k];
        }
        __syncthreads();
    }
}

/* the graph's M at 1 / radius into S.D and S.C: fixed nodes an identity block and no coupling; C[n] = the sum over the edges between n
 * and n + 1, both free, in edge order (the node's incident list), H_ij where i == n and its transpose where i == n + 1 */
template <typename Edge>
__device__ void pg_chain_matrix(const PgGraph<Edge> &G, const PgChain &S, double inv_radius)
{
    for (int n = threadIdx.x; n < G.N; n += PG_THREADS) {
        double *Dn = S.D + (size_t)n * 36, *Cn = S.C + (size_t)n * 36;
        const bool fx = G.fixed[n] != 0;
        for (int k = 0; k < 36; ++k) { Dn[k] = fx ? 0.0 : G.Hd[(size_t)n * 36 + k]; Cn[k] = 0.0; }
        for (int k = 0; k < 6; ++k) Dn[k * 7] = fx ? 1.0 : Dn[k * 7] + G.D[(size_t)n * 6 + k] * inv_radius;
        if (fx || n + 1 >= G.N || G.fixed[n + 1]) continue;
        for (int q = G.inc_off[G.n0 + n]; q < G.inc_off[G.n0 + n + 1]; ++q) {
            if (G.inc_nb[q] != n + 1) continue;
            const int code = G.inc[q], e = code >> 1, side = code & 1;
            const double *Hij = G.eH + (size_t)e * 108;
            if (side == 0) { for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) Cn[a * 6 + b] += Hij[a * 6 + b]; }
            else           { for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) Cn[a * 6 + b] += Hij[b * 6 + a]; }
        }
    }
    __syncthreads();
}

/* Precond: LL_PG_PRECOND_BLOCK_JACOBI (0) is the text as it was; LL_PG_PRECOND_CHAIN (1) factorises M once per LM iteration and applies
 * it once per PCG iteration, block-Jacobi for the iteration where a pivot failed */
template <typename Edge, int Precond>
__global__ __launch_bounds__(PG_THREADS) void k_pg_solve(PgArgs<Edge> A)
{
    __shared__ double sh[8];
    const int tid = threadIdx.x, gi = blockIdx.x;
    const ll_pg_options &o = A.o;
    PgGraph<Edge> G;
    G.n0 = A.node_off[gi]; G.N = A.node_off[gi + 1] - G.n0;
    G.e0 = A.edge_off[gi]; G.E = A.edge_off[gi + 1] - G.e0;
    G.edges = A.edges + G.e0; G.inc_off = A.inc_off; G.inc = A.inc; G.inc_nb = A.inc_nb; G.fixed = A.fixed + G.n0;
    G.x = A.x + (size_t)G.n0 * 7; G.cand = A.cand + (size_t)G.n0 * 7; G.Hd = A.Hd + (size_t)G.n0 * 36;
    G.g = A.g + (size_t)G.n0 * 6; G.D = A.D + (size_t)G.n0 * 6; G.d = A.d + (size_t)G.n0 * 6; G.r = A.r + (size_t)G.n0 * 6;
    G.z = A.z + (size_t)G.n0 * 6; G.p = A.p + (size_t)G.n0 * 6; G.Ap = A.Ap + (size_t)G.n0 * 6;
    G.eH = A.eH + (size_t)G.e0 * 108; G.eg = A.eg + (size_t)G.e0 * 12; G.ecost = A.ecost + G.e0;

    for (int n = tid; n < G.N; n += PG_THREADS) {                  /* quaternions are normalised on entry */
        const double *in = A.pose_in + (size_t)(G.n0 + n) * 7;                  /* ll_pose_unit's operations, kept in place */
        const double qn = sqrt((in[0] * in[0] + in[1] * in[1]) + (in[2] * in[2] + in[3] * in[3]));
        for (int k = 0; k < 4; ++k) G.x[(size_t)n * 7 + k] = in[k] / qn;
        for (int k = 4; k < 7; ++k) G.x[(size_t)n * 7 + k] = in[k];
    }
    __syncthreads();
    double cost = pg_linearise(G, G.x, o, sh);

    if (!A.solve) {
        for (int k = tid; k < G.N * 6; k += PG_THREADS) A.out_nodes[(size_t)G.n0 * 6 + k] = G.g[k];
        if (tid == 0) A.out_cost[gi] = cost;
        return;
    }

    const double cost0 = cost;
    double radius = o.initial_radius, decrease = 2.0, grad_max = 0.0;
    int iterations = 0, successes = 0, n_pcg = 0, term = 3;
    bool lin_ok = true;                                            /* the linearisation at x is finite */
    PgChain S;
    int n_factor = 0, n_fallback = 0;
    if constexpr (Precond == LL_PG_PRECOND_CHAIN) {
        S.N = G.N; S.D = A.cD + (size_t)G.n0 * 36; S.WL = A.cWL + (size_t)G.n0 * 36; S.WR = A.cWR + (size_t)G.n0 * 36;
        S.C = A.cC + (size_t)G.n0 * 36; S.r = A.cr + (size_t)G.n0 * 6;
    }
    for (int iter = 0; iter <= o.max_lm_iterations; ++iter) {     /* every pass below counts one iteration */
        /* ---- can the minimiser continue?  (non-finite, iteration limit, gradient, radius) */
        double gm = 0.0, hs = 0.0;
        for (int n = tid; n < G.N; n += PG_THREADS) {
            if (G.fixed[n]) continue;
            double x2[7], ng[6];
            for (int k = 0; k < 7; ++k) x2[k] = G.x[(size_t)n * 7 + k];
            for (int k = 0; k < 6; ++k) { ng[k] = -G.g[(size_t)n * 6 + k]; hs += G.Hd[(size_t)n * 36 + k * 7]; }     /* a column's squares: inf or NaN if any entry is */
            ll_pose_plus(x2, ng);
            for (int k = 0; k < 7; ++k) { const double dk = fabs(x2[k] - G.x[(size_t)n * 7 + k]); gm = (dk != dk || dk > gm) ? dk : gm; if (gm != gm) break; }
        }
        grad_max = pg_max(gm, sh);
        { double unused = 0.0; pg_sum2(hs, unused, sh); }
        lin_ok = pg_finite(cost) && pg_finite(grad_max) && pg_finite(hs);
        if (!lin_ok) { term = 5; break; }
        if (iter >= o.max_lm_iterations) { term = 3; break; }
        if (grad_max <= o.gradient_tolerance) { term = 0; break; }
        if (radius < o.min_radius) { term = 4; break; }
        ++iterations;

        /* ---- (H + D / radius) d = -g by preconditioned conjugate gradients */
        const double inv_radius = 1.0 / radius;
        double rz = 0.0, gg = 0.0;
        bool chain = false;                                        /* M is factored: this iteration's preconditioner is the chain */
        if constexpr (Precond == LL_PG_PRECOND_CHAIN) {            /* M depends on the radius: once per LM iteration */
            pg_chain_matrix(G, S, inv_radius);
            chain = pg_chain_factor(S, sh);
            ++n_factor;
            if (!chain) ++n_fallback;
            if (chain) {
                for (int k = tid; k < G.N * 6; k += PG_THREADS) S.r[k] = G.fixed[k / 6] ? 0.0 : -G.g[k];
                __syncthreads();
                pg_chain_apply(S, G.z);
            }
        }
        if (chain) {
            for (int n = tid; n < G.N; n += PG_THREADS) {
                const bool fx = G.fixed[n] != 0;
                for (int k = 0; k < 6; ++k) {
                    const double r = -G.g[(size_t)n * 6 + k], z = fx ? 0.0 : G.z[(size_t)n * 6 + k];
                    G.d[(size_t)n * 6 + k] = 0.0; G.r[(size_t)n * 6 + k] = r; G.z[(size_t)n * 6 + k] = z; G.p[(size_t)n * 6 + k] = z;
                    rz += r * z; gg += r * r;
                }
            }
        } else                                                     /* block-Jacobi, the text as it was */
        for (int n = tid; n < G.N; n += PG_THREADS) {
            double r[6], z[6];
            for (int k = 0; k < 6; ++k) { r[k] = -G.g[(size_t)n * 6 + k]; z[k] = 0.0; }
            if (!G.fixed[n]) (void)pg_precondition(G, n, inv_radius, r, z);
            for (int k = 0; k < 6; ++k) {
                G.d[(size_t)n * 6 + k] = 0.0; G.r[(size_t)n * 6 + k] = r[k]; G.z[(size_t)n * 6 + k] = z[k]; G.p[(size_t)n * 6 + k] = z[k];
                rz += r[k] * z[k]; gg += r[k] * r[k];
            }
        }
        pg_sum2(rz, gg, sh);                                       /* its barriers publish p */
        const double stop = o.eta * sqrt(gg);
        for (int k = 0; k < o.max_pcg_iterations; ++k) {
            pg_matvec(G, G.p, G.Ap, inv_radius);
            double pAp = 0.0, unused = 0.0;
            for (int n = tid; n < G.N; n += PG_THREADS)
                for (int a = 0; a < 6; ++a) pAp += G.p[(size_t)n * 6 + a] * G.Ap[(size_t)n * 6 + a];
            pg_sum2(pAp, unused, sh);
            if (!(pAp > 0.0) || !pg_finite(pAp) || !pg_finite(rz)) break;
            const double alpha = rz / pAp;
            double rr = 0.0, rz2 = 0.0;
            if (chain) {
                for (int n = tid; n < G.N; n += PG_THREADS)
                    for (int a = 0; a < 6; ++a) {
                        G.d[(size_t)n * 6 + a] += alpha * G.p[(size_t)n * 6 + a];
                        const double r = G.r[(size_t)n * 6 + a] - alpha * G.Ap[(size_t)n * 6 + a];
                        G.r[(size_t)n * 6 + a] = r; S.r[(size_t)n * 6 + a] = G.fixed[n] ? 0.0 : r;
                        rr += r * r;
                    }
                __syncthreads();
                pg_chain_apply(S, G.z);
                for (int n = tid; n < G.N; n += PG_THREADS) {
                    const bool fx = G.fixed[n] != 0;
                    for (int a = 0; a < 6; ++a) {
                        const double z = fx ? 0.0 : G.z[(size_t)n * 6 + a];
                        G.z[(size_t)n * 6 + a] = z; rz2 += G.r[(size_t)n * 6 + a] * z;
                    }
                }
            } else                                                 /* block-Jacobi, the text as it was */
            for (int n = tid; n < G.N; n += PG_THREADS) {
                double r[6], z[6];
                for (int a = 0; a < 6; ++a) {
                    G.d[(size_t)n * 6 + a] += alpha * G.p[(size_t)n * 6 + a];
                    r[a] = G.r[(size_t)n * 6 + a] - alpha * G.Ap[(size_t)n * 6 + a];
                    G.r[(size_t)n * 6 + a] = r[a]; z[a] = 0.0;
                }
                if (!G.fixed[n]) (void)pg_precondition(G, n, inv_radius, r, z);
                for (int a = 0; a < 6; ++a) { G.z[(size_t)n * 6 + a] = z[a]; rr += r[a] * r[a]; rz2 += r[a] * z[a]; }
            }
            pg_sum2(rr, rz2, sh);
            ++n_pcg;
            if (!(sqrt(rr) > stop)) break;                         /* converged (inexact Newton), or a NaN */
            const double beta = rz2 / rz;
            rz = rz2;
            for (int n = tid; n < G.N; n += PG_THREADS)
                for (int a = 0; a < 6; ++a) G.p[(size_t)n * 6 + a] = G.z[(size_t)n * 6 + a] + beta * G.p[(size_t)n * 6 + a];
            __syncthreads();
        }

        /* ---- the model's cost change, -(g.d + d.H d / 2), H without the damping */
        __syncthreads();
        pg_matvec(G, G.d, G.Ap, 0.0);
        double gd = 0.0, dHd = 0.0;
        for (int n = tid; n < G.N; n += PG_THREADS)
            for (int a = 0; a < 6; ++a) { const double da = G.d[(size_t)n * 6 + a]; gd += G.g[(size_t)n * 6 + a] * da; dHd += da * G.Ap[(size_t)n * 6 + a]; }
        pg_sum2(gd, dHd, sh);
        const double mcc = -(gd + 0.5 * dHd);
        if (!(mcc > 0.0) || !pg_finite(mcc)) { radius *= 0.5; continue; }          /* invalid step */

        /* ---- the candidate, the parameter test, its cost */
        double step2 = 0.0, x2n = 0.0;
        for (int n = tid; n < G.N; n += PG_THREADS) {
            double c7[7];
            for (int k = 0; k < 7; ++k) c7[k] = G.x[(size_t)n * 7 + k];
            if (!G.fixed[n]) ll_pose_plus(c7, G.d + (size_t)n * 6);
            for (int k = 0; k < 7; ++k) {
                const double xk = G.x[(size_t)n * 7 + k], ek = c7[k] - xk;
                G.cand[(size_t)n * 7 + k] = c7[k]; step2 += ek * ek; x2n += xk * xk;
            }
        }
        pg_sum2(step2, x2n, sh);                                   /* its barriers publish cand */
        if (!pg_finite(step2)) { term = 5; break; }
        if (sqrt(step2) <= o.parameter_tolerance * (sqrt(x2n) + o.parameter_tolerance)) { term = 2; break; }
        double cc = 0.0, unused = 0.0;
        for (int e = tid; e < G.E; e += PG_THREADS) {
            const Edge &ed = G.edges[e];
            cc += pg_edge_cost(G.cand + (size_t)ed.i * 7, G.cand + (size_t)ed.j * 7, ed);
        }
        pg_sum2(cc, unused, sh);
        if (!pg_finite(cc)) { term = 5; break; }
        if (fabs(cost - cc) <= o.function_tolerance * cost) { term = 1; break; }

        /* ---- accept or reject */
        const double rho = (cost - cc) / mcc;
        if (rho > o.min_relative_decrease) {
            for (int k = tid; k < G.N * 7; k += PG_THREADS) G.x[k] = G.cand[k];
            __syncthreads();
            (void)pg_linearise(G, G.x, o, sh);
            cost = cc;
            const double f = 1.0 - pow(2.0 * rho - 1.0, 3.0);
            radius = fmin(radius / fmax(1.0 / 3.0, f), o.max_radius);
            decrease = 2.0; ++successes;
        } else {
            radius = radius / decrease;
            decrease *= 2.0;
        }
    }

    __syncthreads();
    for (int k = tid; k < G.N * 7; k += PG_THREADS) A.out_nodes[(size_t)G.n0 * 7 + k] = G.x[k];
    if (tid == 0) {
        ll_pg_record R;
        R.cost0 = cost0; R.cost = cost; R.grad_max = grad_max;
        R.lm_iterations = iterations; R.lm_successes = successes; R.pcg_iterations = n_pcg; R.termination = term;
        A.rec[gi] = R;
        if constexpr (Precond == LL_PG_PRECOND_CHAIN) { A.cstat[gi * 2] = n_factor; A.cstat[gi * 2 + 1] = n_fallback; }
    }
}

/* ll_posegraphs_chain_solve: system = blockIdx.x; its diagonal blocks, couplings and right-hand side are in the workspace's D, C and r */
__global__ __launch_bounds__(PG_THREADS) void k_pg_chain_solve(const int *node_off, double *cD, double *cWL, double *cWR, double *cC, double *cr,
                                                               double *cz, int *status)
{
    __shared__ double sh[8];
    const int n0 = node_off[blockIdx.x];
    PgChain S;
    S.N = node_off[blockIdx.x + 1] - n0;
    S.D = cD + (size_t)n0 * 36; S.WL = cWL + (size_t)n0 * 36; S.WR = cWR + (size_t)n0 * 36; S.C = cC + (size_t)n0 * 36; S.r = cr + (size_t)n0 * 6;
    double *z = cz + (size_t)n0 * 6;
    if (S.N < 1) { if (threadIdx.x == 0) status[blockIdx.x] = 0; return; }
    const bool ok = pg_chain_factor(S, sh);
    if (ok) pg_chain_apply(S, z);
    else for (int k = threadIdx.x; k < S.N * 6; k += PG_THREADS) z[k] = 0.0;
    if (threadIdx.x == 0) status[blockIdx.x] = ok ? 0 : 1;
}

/* ------------------------------------------------------------------ device: covariances (ll_posegraphs_covariances; the contract is in the header)
 * Sigma = H^-1 with H the matrix of pg_matvec at damp 0, at the poses of the call.  Three launches:
 *   k_pg_cov_prepare   a workgroup per graph that has a query: normalise, pg_linearise into the solves' workspace, and under the chain
 *                      preconditioner pg_chain_matrix at 1 / radius = 0 and pg_chain_factor, once per graph; a flag per graph for a failed pivot.
 *   k_pg_cov_columns   a workgroup per (source, k): H x = e_(node, k) by the PCG of k_pg_solve.  Hd, eH, D and the chain's factors are shared
 *                      and only read; d, r, z, p, Ap and the chain's r are the column's own rows (36 doubles per node of the graph).
 *                      pg_chain_apply writes S.r and z and nothing else, which is what lets the columns of a graph share its factors.
 *   k_pg_cov_gather    a small workgroup per query puts the 12 x 12 together from the columns' d.
 * A column depends on its graph alone: every index is relative to the graph, every sum has a fixed shape. */
struct PgCovSource { long long row; int graph, node, n, pad; };   /* row: the first of the source's 6 n rows; node local to the graph of n nodes */
struct PgCovQuery { int sa, sb, a, b; };                           /* the sources of a and b (-1: fixed, or no b), the nodes */

template <typename Edge>
__device__ __forceinline__ void pg_cov_graph(const PgArgs<Edge> &A, int gi, PgGraph<Edge> &G)
{
    G.n0 = A.node_off[gi]; G.N = A.node_off[gi + 1] - G.n0;
    G.e0 = A.edge_off[gi]; G.E = A.edge_off[gi + 1] - G.e0;
    G.edges = A.edges + G.e0; G.inc_off = A.inc_off; G.inc = A.inc; G.inc_nb = A.inc_nb; G.fixed = A.fixed + G.n0;
    G.x = A.x + (size_t)G.n0 * 7; G.cand = A.cand + (size_t)G.n0 * 7; G.Hd = A.Hd + (size_t)G.n0 * 36;
    G.g = A.g + (size_t)G.n0 * 6; G.D = A.D + (size_t)G.n0 * 6; G.d = A.d + (size_t)G.n0 * 6; G.r = A.r + (size_t)G.n0 * 6;
    G.z = A.z + (size_t)G.n0 * 6; G.p = A.p + (size_t)G.n0 * 6; G.Ap = A.Ap + (size_t)G.n0 * 6;
    G.eH = A.eH + (size_t)G.e0 * 108; G.eg = A.eg + (size_t)G.e0 * 12; G.ecost = A.ecost + G.e0;
}

template <typename Edge, int Precond>
__global__ __launch_bounds__(PG_THREADS) void k_pg_cov_prepare(PgArgs<Edge> A, const int *graphs, int *flags)
{
    __shared__ double sh[8];
    const int tid = threadIdx.x, gi = graphs[blockIdx.x];
    PgGraph<Edge> G;
    pg_cov_graph(A, gi, G);
    for (int n = tid; n < G.N; n += PG_THREADS) {                  /* quaternions are normalised on entry */
        const double *in = A.pose_in + (size_t)(G.n0 + n) * 7;                  /* ll_pose_unit's operations, kept in place */
        const double qn = sqrt((in[0] * in[0] + in[1] * in[1]) + (in[2] * in[2] + in[3] * in[3]));
        for (int k = 0; k < 4; ++k) G.x[(size_t)n * 7 + k] = in[k] / qn;
        for (int k = 4; k < 7; ++k) G.x[(size_t)n * 7 + k] = in[k];
    }
    __syncthreads();
    (void)pg_linearise(G, G.x, A.o, sh);
    bool ok = true;
    if constexpr (Precond == LL_PG_PRECOND_CHAIN) {
        PgChain S;
        S.N = G.N; S.D = A.cD + (size_t)G.n0 * 36; S.WL = A.cWL + (size_t)G.n0 * 36; S.WR = A.cWR + (size_t)G.n0 * 36;
        S.C = A.cC + (size_t)G.n0 * 36; S.r = A.cr + (size_t)G.n0 * 6;
        pg_chain_matrix(G, S, 0.0);
        ok = pg_chain_factor(S, sh);
    }
    if (tid == 0) flags[gi] = ok ? 0 : 1;
}

template <typename Edge, int Precond>
__global__ __launch_bounds__(PG_THREADS) void k_pg_cov_columns(PgArgs<Edge> A, const PgCovSource *src, const int *flags, double *rows,
                                                               ll_pg_cov_record *col, int max_iterations, double tolerance)
{
    __shared__ double sh[8];
    const int tid = threadIdx.x, k = blockIdx.x % 6;
    const PgCovSource sc = src[blockIdx.x / 6];
    PgGraph<Edge> G;
    pg_cov_graph(A, sc.graph, G);
    const size_t N6 = (size_t)G.N * 6;
    double *w = rows + ((size_t)sc.row + (size_t)k * G.N) * 36;   /* the column's own rows */
    G.d = w; G.r = w + N6; G.z = w + 2 * N6; G.p = w + 3 * N6; G.Ap = w + 4 * N6;
    PgChain S;
    bool chain = false;
    if constexpr (Precond == LL_PG_PRECOND_CHAIN) {
        S.N = G.N; S.D = A.cD + (size_t)G.n0 * 36; S.WL = A.cWL + (size_t)G.n0 * 36; S.WR = A.cWR + (size_t)G.n0 * 36;
        S.C = A.cC + (size_t)G.n0 * 36; S.r = w + 5 * N6;
        chain = flags[sc.graph] == 0;                              /* a failed pivot: block-Jacobi for the graph's columns */
    }
    const int unit = sc.node * 6 + k;

    double rz = 0.0, unused = 0.0;
    if (chain) {
        for (int i = tid; i < G.N * 6; i += PG_THREADS) S.r[i] = i == unit ? 1.0 : 0.0;
        __syncthreads();
        pg_chain_apply(S, G.z);
        for (int n = tid; n < G.N; n += PG_THREADS) {
            const bool fx = G.fixed[n] != 0;
            for (int a = 0; a < 6; ++a) {
                const double r = n * 6 + a == unit ? 1.0 : 0.0, z = fx ? 0.0 : G.z[(size_t)n * 6 + a];
                G.d[(size_t)n * 6 + a] = 0.0; G.r[(size_t)n * 6 + a] = r; G.z[(size_t)n * 6 + a] = z; G.p[(size_t)n * 6 + a] = z;
                rz += r * z;
            }
        }
    } else
    for (int n = tid; n < G.N; n += PG_THREADS) {
        double r[6], z[6];
        for (int a = 0; a < 6; ++a) { r[a] = n * 6 + a == unit ? 1.0 : 0.0; z[a] = 0.0; }
        if (!G.fixed[n]) (void)pg_precondition(G, n, 0.0, r, z);
        for (int a = 0; a < 6; ++a) {
            G.d[(size_t)n * 6 + a] = 0.0; G.r[(size_t)n * 6 + a] = r[a]; G.z[(size_t)n * 6 + a] = z[a]; G.p[(size_t)n * 6 + a] = z[a];
            rz += r[a] * z[a];
        }
    }
    pg_sum2(rz, unused, sh);                                       /* its barriers publish p */

    double rnorm = 1.0;                                            /* |e_(node, k)| */
    int it = 0, status;
    for (;;) {
        if (rnorm <= tolerance) { status = 0; break; }
        if (it >= max_iterations) { status = 1; break; }
        pg_matvec(G, G.p, G.Ap, 0.0);
        double pAp = 0.0;
        unused = 0.0;
        for (int n = tid; n < G.N; n += PG_THREADS)
            for (int a = 0; a < 6; ++a) pAp += G.p[(size_t)n * 6 + a] * G.Ap[(size_t)n * 6 + a];
        pg_sum2(pAp, unused, sh);
        if (!(pAp > 0.0) || !pg_finite(pAp) || !pg_finite(rz)) { status = 2; break; }
        const double alpha = rz / pAp;
        double rr = 0.0, rz2 = 0.0;
        if (chain) {
            for (int n = tid; n < G.N; n += PG_THREADS)
                for (int a = 0; a < 6; ++a) {
                    G.d[(size_t)n * 6 + a] += alpha * G.p[(size_t)n * 6 + a];
                    const double r = G.r[(size_t)n * 6 + a] - alpha * G.Ap[(size_t)n * 6 + a];
                    G.r[(size_t)n * 6 + a] = r; S.r[(size_t)n * 6 + a] = G.fixed[n] ? 0.0 : r;
                    rr += r * r;
                }
            __syncthreads();
            pg_chain_apply(S, G.z);
            for (int n = tid; n < G.N; n += PG_THREADS) {
                const bool fx = G.fixed[n] != 0;
                for (int a = 0; a < 6; ++a) {
                    const double z = fx ? 0.0 : G.z[(size_t)n * 6 + a];
                    G.z[(size_t)n * 6 + a] = z; rz2 += G.r[(size_t)n * 6 + a] * z;
                }
            }
        } else
        for (int n = tid; n < G.N; n += PG_THREADS) {
            double r[6], z[6];
            for (int a = 0; a < 6; ++a) {
                G.d[(size_t)n * 6 + a] += alpha * G.p[(size_t)n * 6 + a];
                r[a] = G.r[(size_t)n * 6 + a] - alpha * G.Ap[(size_t)n * 6 + a];
                G.r[(size_t)n * 6 + a] = r[a]; z[a] = 0.0;
            }
            if (!G.fixed[n]) (void)pg_precondition(G, n, 0.0, r, z);
            for (int a = 0; a < 6; ++a) { G.z[(size_t)n * 6 + a] = z[a]; rr += r[a] * r[a]; rz2 += r[a] * z[a]; }
        }
        pg_sum2(rr, rz2, sh);
        ++it;
        if (!pg_finite(rr)) { status = 2; break; }
        rnorm = sqrt(rr);
        const double beta = rz2 / rz;
        rz = rz2;
        for (int n = tid; n < G.N; n += PG_THREADS)
            for (int a = 0; a < 6; ++a) G.p[(size_t)n * 6 + a] = G.z[(size_t)n * 6 + a] + beta * G.p[(size_t)n * 6 + a];
        __syncthreads();
    }
    if (tid == 0) {
        ll_pg_cov_record R;
        R.status = status; R.pcg_iterations = it; R.residual = rnorm;
        col[blockIdx.x] = R;
    }
}

/* query = blockIdx.x, 64 threads over the 144 entries.  Sigma[(m, c)][(n, k)] is entry (m, c) of column k of source n; the diagonal
 * blocks are symmetrised, the cross block is read from the columns of the smaller node index whichever way round the query names them */
__global__ __launch_bounds__(64) void k_pg_cov_gather(const PgCovQuery *qry, const PgCovSource *src, const double *rows,
                                                      const ll_pg_cov_record *col, double *joint, ll_pg_cov_record *rec)
{
    const PgCovQuery q = qry[blockIdx.x];
    int status = 0, iterations = 0;
    double residual = 0.0;
    for (int side = 0; side < 2; ++side) {
        const int s = side ? q.sb : q.sa;
        if (s < 0 || (side && s == q.sa)) continue;
        for (int k = 0; k < 6; ++k) {
            const ll_pg_cov_record c = col[s * 6 + k];
            status = c.status > status ? c.status : status; iterations += c.pcg_iterations; residual = pg_max2(residual, c.residual);
        }
    }
    const double *da = nullptr, *db = nullptr;                     /* column k of a source: + k * n * 36, entry (m, c): + m * 6 + c */
    size_t stride = 0;
    if (q.sa >= 0) { const PgCovSource s = src[q.sa]; da = rows + (size_t)s.row * 36; stride = (size_t)s.n * 36; }
    if (q.sb >= 0) { const PgCovSource s = src[q.sb]; db = rows + (size_t)s.row * 36; stride = (size_t)s.n * 36; }
    for (int t = threadIdx.x; t < 144; t += 64) {
        const int R = t / 12, Cc = t % 12, br = R / 6, bc = Cc / 6, c = R % 6, k = Cc % 6;
        double v = 0.0;
        if (status != 2) {
            if (br == 0 && bc == 0) { if (da) v = 0.5 * (da[k * stride + q.a * 6 + c] + da[c * stride + q.a * 6 + k]); }
            else if (br == 1 && bc == 1) { if (db) v = 0.5 * (db[k * stride + q.b * 6 + c] + db[c * stride + q.b * 6 + k]); }
            else if (da && db) {
                const bool a_low = q.a < q.b;
                const double *lo = a_low ? da : db;
                const int hi = a_low ? q.b : q.a;
                /* (br, bc) = (0, 1) is S_ab; with a low it is the transpose of what a's columns hold at b, with b low what b's hold at a */
                const bool direct = (br == 1) == a_low;
                v = direct ? lo[k * stride + hi * 6 + c] : lo[c * stride + hi * 6 + k];
            }
        }
        joint[(size_t)blockIdx.x * 144 + t] = v;
    }
    if (threadIdx.x == 0) {
        ll_pg_cov_record r;
        r.status = status; r.pcg_iterations = iterations; r.residual = residual;
        rec[blockIdx.x] = r;
    }
}

/* ------------------------------------------------------------------ host side */
static int pg_fail(ll_posegraphs *pg, int code, const std::string &what) { pg->err = "posegraphs: " + what; return code; }

#define PG_HIP(call) LL_HIP_CHECK(pg_fail, pg, "", call, #call)

static size_t pg_up8(size_t b) { return (b + 7) & ~(size_t)7; }

/* the byte offsets of the sections of the upload for (graphs, nodes, edges); [8] = the total */
static void pg_in_layout(size_t G, size_t N, size_t E, size_t edge_bytes, size_t off[9])
{
    const size_t sz[8] = {N * 7 * sizeof(double), E * edge_bytes, (G + 1) * sizeof(int), (G + 1) * sizeof(int),
                          (N + 1) * sizeof(int), 2 * E * sizeof(int), 2 * E * sizeof(int), N};
    off[0] = 0;
    for (int k = 0; k < 8; ++k) off[k + 1] = off[k] + pg_up8(sz[k]);
}

extern "C" void ll_pg_default_options(ll_pg_options *o)
{
    if (!o) return;
    o->max_lm_iterations = 50; o->max_pcg_iterations = 1000; o->eta = 0.1;
    o->initial_radius = 1e4; o->max_radius = 1e16; o->min_radius = 1e-32;
    o->min_relative_decrease = 1e-3; o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
    o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
}

extern "C" void ll_posegraphs_destroy(ll_posegraphs *pg)
{
    if (!pg) return;
    (void)hipSetDevice(pg->ctx->device);
    for (void *p : {(void *)pg->d_in, (void *)pg->d_out, (void *)pg->d_ws, (void *)pg->d_chain, (void *)pg->d_cov}) if (p) (void)hipFree(p);
    for (hipEvent_t e : pg->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : pg->cov_ev) if (e) (void)hipEventDestroy(e);
    delete pg;
}

extern "C" int ll_posegraphs_create(ll_ctx *ctx, int max_graphs, int max_nodes_total, int max_edges_total, ll_posegraphs **out)
{
    if (!ctx || !out) return LL_ERR_ARG;
    *out = nullptr;
    if (max_graphs < 1 || max_nodes_total < 1 || max_edges_total < 0 || max_graphs > (1 << 20) || max_nodes_total > (1 << 26) || max_edges_total > (1 << 26)) {
        ctx->err = "posegraphs: max_graphs outside 1 .. 2^20, max_nodes_total outside 1 .. 2^26 or max_edges_total outside 0 .. 2^26";
        return LL_ERR_ARG;
    }
    LL_HIP(hipSetDevice(ctx->device));
    ll_posegraphs *pg = new ll_posegraphs();
    pg->ctx = ctx; pg->max_graphs = max_graphs; pg->max_nodes = max_nodes_total; pg->max_edges = max_edges_total;
    const size_t G = (size_t)max_graphs, N = (size_t)max_nodes_total, E = (size_t)max_edges_total;
    size_t off[9];
    pg_in_layout(G, N, E, sizeof(ll_pg_edge6), off);              /* room for either edge type */
    pg->in_bytes = off[8];
    pg->out_bytes = N * 7 * sizeof(double) + G * sizeof(ll_pg_record);
    const size_t ws_bytes = (N * PG_NODE_DOUBLES + E * PG_EDGE_DOUBLES + 1) * sizeof(double);
    bool ok = hipMalloc((void **)&pg->d_in, pg->in_bytes) == hipSuccess && hipMalloc((void **)&pg->d_out, pg->out_bytes) == hipSuccess &&
              hipMalloc((void **)&pg->d_ws, ws_bytes) == hipSuccess;
    for (hipEvent_t &e : pg->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ll_posegraphs_destroy(pg);
        ctx->err = "posegraphs: allocation failed (" + std::to_string(off[8] + ws_bytes) + " bytes)";
        return LL_ERR_HIP;
    }
    *out = pg;
    return LL_OK;
}

extern "C" const char *ll_posegraphs_last_error(const ll_posegraphs *pg) { return pg ? pg->err.c_str() : "posegraphs: NULL handle"; }

/* the chain preconditioner's workspace for max_nodes and max_graphs: per node the factored block, both W and the coupling (36 doubles
 * each), the right-hand side and z of ll_posegraphs_chain_solve (6 each); per graph the offsets and status of chain_solve and 2 counts */
struct PgChainWs { double *D, *WL, *WR, *C, *r, *z; int *node_off, *stat, *status; size_t bytes; };

static PgChainWs pg_chain_ws(const ll_posegraphs *pg)
{
    const size_t N = (size_t)pg->max_nodes, G = (size_t)pg->max_graphs;
    PgChainWs w;
    double *d = pg->d_chain;
    w.D = d; d += N * 36; w.WL = d; d += N * 36; w.WR = d; d += N * 36; w.C = d; d += N * 36; w.r = d; d += N * 6; w.z = d; d += N * 6;
    int *i = (int *)d;
    w.node_off = i; i += G + 1; w.stat = i; i += 2 * G; w.status = i; i += G;
    w.bytes = N * 156 * sizeof(double) + (4 * G + 1) * sizeof(int);
    return w;
}

static int pg_chain_alloc(ll_posegraphs *pg)
{
    if (pg->d_chain) return LL_OK;
    const size_t bytes = pg_chain_ws(pg).bytes;
    if (hipSetDevice(pg->ctx->device) != hipSuccess || hipMalloc((void **)&pg->d_chain, bytes) != hipSuccess) {
        (void)hipGetLastError();
        pg->d_chain = nullptr;
        return pg_fail(pg, LL_ERR_HIP, "the chain preconditioner's workspace could not be allocated (" + std::to_string(bytes) + " bytes)");
    }
    return LL_OK;
}

extern "C" int ll_posegraphs_set_preconditioner(ll_posegraphs *pg, int kind)
{
    if (!pg) return LL_ERR_ARG;
    if (kind != LL_PG_PRECOND_BLOCK_JACOBI && kind != LL_PG_PRECOND_CHAIN)
        return pg_fail(pg, LL_ERR_ARG, "set_preconditioner: kind " + std::to_string(kind) + " is neither LL_PG_PRECOND_BLOCK_JACOBI nor LL_PG_PRECOND_CHAIN");
    if (kind == LL_PG_PRECOND_CHAIN) { const int rc = pg_chain_alloc(pg); if (rc) return rc; }
    pg->precond = kind;
    return LL_OK;
}

extern "C" int ll_posegraphs_preconditioner(const ll_posegraphs *pg) { return pg ? pg->precond : LL_ERR_ARG; }

/* counts2: factorisations of M, and LM iterations that fell back to block-Jacobi, over the graphs of the last solve */
extern "C" int ll_posegraphs_precond_stats(ll_posegraphs *pg, long long counts2[2])
{
    if (!pg || !counts2) return LL_ERR_ARG;
    counts2[0] = pg->pc_counts[0]; counts2[1] = pg->pc_counts[1];
    return LL_OK;
}

static int pg_check_options(ll_posegraphs *pg, const ll_pg_options &o)
{
    const double v[10] = {o.eta, o.initial_radius, o.max_radius, o.min_radius, o.min_relative_decrease, o.min_lm_diagonal, o.max_lm_diagonal,
                          o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance};
    bool ok = o.max_lm_iterations >= 0 && o.max_pcg_iterations >= 1 && ll_finite_n(v, 10);
    ok = ok && o.eta > 0.0 && o.eta < 1.0 && o.initial_radius > 0.0 && o.max_radius >= o.initial_radius && o.min_radius >= 0.0 &&
         o.min_relative_decrease >= 0.0 && o.min_relative_decrease < 1.0 && o.min_lm_diagonal > 0.0 && o.max_lm_diagonal >= o.min_lm_diagonal &&
         o.function_tolerance >= 0.0 && o.gradient_tolerance >= 0.0 && o.parameter_tolerance >= 0.0;
    return ok ? LL_OK : pg_fail(pg, LL_ERR_ARG, "options out of range (iterations >= 0 / >= 1, 0 < eta < 1, 0 < initial_radius <= max_radius, "
                                                "0 < min_lm_diagonal <= max_lm_diagonal, tolerances >= 0, all finite)");
}

static bool pg_finite_weights(const ll_pg_edge &e) { return ll_finite_n(e.sqrt_info, 6); }
static bool pg_finite_weights(const ll_pg_edge6 &e) { return ll_finite_n(e.S, 36); }

/* the checks every call shares, in two parts (a call's own checks of its outputs and options lie between them): the layout ... */
template <typename Edge>
static int pg_check_layout(ll_posegraphs *pg, const char *who, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                           const Edge *edges)
{
    auto bad = [&](int code, const std::string &what) { return pg_fail(pg, code, who + what); };
    if (n_graphs < 0 || !node_off || !edge_off) return bad(LL_ERR_ARG, "n_graphs < 0, or node_off / edge_off is NULL");
    if (n_graphs > pg->max_graphs) return bad(LL_ERR_CAPACITY, std::to_string(n_graphs) + " graphs exceed max_graphs " + std::to_string(pg->max_graphs));
    if (node_off[0] != 0 || edge_off[0] != 0) return bad(LL_ERR_ARG, "offsets must start at 0");
    for (int g = 0; g < n_graphs; ++g)
        if (node_off[g + 1] < node_off[g] || edge_off[g + 1] < edge_off[g]) return bad(LL_ERR_ARG, "graph " + std::to_string(g) + ": offsets do not ascend");
    const int N = node_off[n_graphs], E = edge_off[n_graphs];
    if (N > pg->max_nodes) return bad(LL_ERR_CAPACITY, std::to_string(N) + " nodes exceed max_nodes_total " + std::to_string(pg->max_nodes));
    if (E > pg->max_edges) return bad(LL_ERR_CAPACITY, std::to_string(E) + " edges exceed max_edges_total " + std::to_string(pg->max_edges));
    if ((N > 0 && !poses_w7) || (E > 0 && !edges)) return bad(LL_ERR_ARG, "poses or edges is NULL");
    return LL_OK;
}

/* ... and every graph's poses, fixed node and edges */
template <typename Edge>
static int pg_check_graphs(ll_posegraphs *pg, const char *who, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                           const unsigned char *fixed, const Edge *edges)
{
    auto bad = [&](int code, const std::string &what) { return pg_fail(pg, code, who + what); };
    for (int g = 0; g < n_graphs; ++g) {
        const int n0 = node_off[g], n = node_off[g + 1] - n0;
        const std::string gs = "graph " + std::to_string(g);
        bool any_fixed = !fixed && n > 0;
        for (int k = 0; k < n; ++k) {
            const double *p = poses_w7 + (size_t)(n0 + k) * 7;
            if (!ll_finite_n(p, 7)) return bad(LL_ERR_ARG, gs + ", node " + std::to_string(k) + ": the pose is not finite");
            if (ll_zero_quat(p)) return bad(LL_ERR_ARG, gs + ", node " + std::to_string(k) + ": zero quaternion");
            if (fixed && fixed[n0 + k]) any_fixed = true;
        }
        if (!any_fixed) return bad(LL_ERR_ARG, gs + " has no fixed node");
        for (int e = edge_off[g]; e < edge_off[g + 1]; ++e) {
            const Edge &ed = edges[e];
            const std::string es = gs + ", edge " + std::to_string(e - edge_off[g]);
            if (ed.i < 0 || ed.i >= n || ed.j < 0 || ed.j >= n) return bad(LL_ERR_ARG, es + ": a node index lies outside the graph");
            if (ed.i == ed.j) return bad(LL_ERR_ARG, es + ": i == j");
            if (!ll_finite_n(ed.Z_w7, 7) || !pg_finite_weights(ed) || !std::isfinite(ed.huber)) return bad(LL_ERR_ARG, es + ": the measurement or a weight is not finite");
            if (ll_zero_quat(ed.Z_w7)) return bad(LL_ERR_ARG, es + ": zero quaternion");
        }
    }
    return LL_OK;
}

/* the upload of a call in page-locked memory at `pin`, laid out by `off` (pg_in_layout): poses, edges, offsets, the node -> incident-edge
 * lists (edge order), fixed */
struct PgPacked { int *inc_off, *inc, *inc_nb; unsigned char *fx; };

template <typename Edge>
static PgPacked pg_pack(unsigned char *pin, const size_t off[9], int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                        const unsigned char *fixed, const Edge *edges)
{
    const int N = node_off[n_graphs], E = edge_off[n_graphs];
    if (N > 0) std::memcpy(pin + off[0], poses_w7, (size_t)N * 7 * sizeof(double));
    if (E > 0) std::memcpy(pin + off[1], edges, (size_t)E * sizeof(Edge));
    std::memcpy(pin + off[2], node_off, (size_t)(n_graphs + 1) * sizeof(int));
    std::memcpy(pin + off[3], edge_off, (size_t)(n_graphs + 1) * sizeof(int));
    int *inc_off = (int *)(pin + off[4]), *inc = (int *)(pin + off[5]), *inc_nb = (int *)(pin + off[6]);
    unsigned char *fx = pin + off[7];
    for (int k = 0; k <= N; ++k) inc_off[k] = 0;
    for (int g = 0; g < n_graphs; ++g)
        for (int e = edge_off[g]; e < edge_off[g + 1]; ++e) { ++inc_off[node_off[g] + edges[e].i + 1]; ++inc_off[node_off[g] + edges[e].j + 1]; }
    for (int k = 0; k < N; ++k) inc_off[k + 1] += inc_off[k];
    {
        std::vector<int> fill(inc_off, inc_off + N);
        for (int g = 0; g < n_graphs; ++g)
            for (int e = edge_off[g]; e < edge_off[g + 1]; ++e) {                  /* ascending e: every node's list is in edge order */
                const int le = e - edge_off[g], i = edges[e].i, j = edges[e].j;
                int q = fill[node_off[g] + i]++; inc[q] = le * 2; inc_nb[q] = j;
                q = fill[node_off[g] + j]++;     inc[q] = le * 2 + 1; inc_nb[q] = i;
            }
    }
    for (int g = 0; g < n_graphs; ++g)
        for (int k = node_off[g]; k < node_off[g + 1]; ++k) fx[k] = fixed ? (fixed[k] ? 1 : 0) : (k == node_off[g] ? 1 : 0);
    PgPacked P = {inc_off, inc, inc_nb, fx};
    return P;
}

/* the kernels' view of the upload in d_in and of the workspace, for a call of N nodes and E edges */
template <typename Edge>
static void pg_device_views(const ll_posegraphs *pg, const size_t off[9], size_t Nn, size_t En, PgArgs<Edge> &A)
{
    A.pose_in = (const double *)(pg->d_in + off[0]); A.edges = (const Edge *)(pg->d_in + off[1]);
    A.node_off = (const int *)(pg->d_in + off[2]); A.edge_off = (const int *)(pg->d_in + off[3]);
    A.inc_off = (const int *)(pg->d_in + off[4]); A.inc = (const int *)(pg->d_in + off[5]); A.inc_nb = (const int *)(pg->d_in + off[6]);
    A.fixed = pg->d_in + off[7];
    double *w = pg->d_ws;
    A.x = w; w += Nn * 7; A.cand = w; w += Nn * 7; A.Hd = w; w += Nn * 36; A.g = w; w += Nn * 6; A.D = w; w += Nn * 6; A.d = w; w += Nn * 6;
    A.r = w; w += Nn * 6; A.z = w; w += Nn * 6; A.p = w; w += Nn * 6; A.Ap = w; w += Nn * 6;
    A.eH = w; w += En * 108; A.eg = w; w += En * 12; A.ecost = w;
}

/* validate the call, pack it into page-locked scratch, enqueue the upload and the launch, download, synchronise ONCE */
template <typename Edge>
static int pg_run(ll_posegraphs *pg, bool solve, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                  const unsigned char *fixed, const Edge *edges, const ll_pg_options *opt, double *out_a, void *out_b)
{
    if (!pg) return LL_ERR_ARG;
    const char *who = solve ? "solve: " : "evaluate: ";
    auto bad = [&](int code, const std::string &what) { return pg_fail(pg, code, who + what); };
    { const int rc = pg_check_layout(pg, who, n_graphs, node_off, edge_off, poses_w7, edges); if (rc) return rc; }
    const int N = node_off[n_graphs], E = edge_off[n_graphs];
    if (solve ? false : (n_graphs > 0 && (!out_a || (N > 0 && !out_b)))) return bad(LL_ERR_ARG, "cost or grad6 is NULL");
    ll_pg_options o;
    ll_pg_default_options(&o);
    if (opt) o = *opt;
    if (solve) { const int rc = pg_check_options(pg, o); if (rc) return rc; }
    { const int rc = pg_check_graphs(pg, who, n_graphs, node_off, edge_off, poses_w7, fixed, edges); if (rc) return rc; }
    pg->counts[0] = n_graphs; pg->counts[1] = pg->counts[2] = 0;
    pg->ms[solve ? 1 : 0] = 0.0;
    if (solve) pg->pc_counts[0] = pg->pc_counts[1] = 0;
    if (n_graphs == 0) return LL_OK;
    const bool chain = solve && pg->precond == LL_PG_PRECOND_CHAIN;                /* evaluate solves nothing */

    /* ---- pack: poses, edges, offsets, the node -> incident-edge lists (edge order), fixed */
    size_t off[9];
    pg_in_layout((size_t)n_graphs, (size_t)N, (size_t)E, sizeof(Edge), off);
    const size_t per_node = solve ? 7 : 6;
    const size_t out_b_bytes = solve ? (size_t)n_graphs * sizeof(ll_pg_record) : (size_t)n_graphs * sizeof(double);
    const size_t down = (size_t)N * per_node * sizeof(double) + out_b_bytes;
    const size_t stat_bytes = chain ? (size_t)n_graphs * 2 * sizeof(int) : 0;
    unsigned char *pin = (unsigned char *)ll_pinned_scratch(off[8] + pg_up8(down) + stat_bytes);
    if (!pin) return bad(LL_ERR_HIP, "no page-locked scratch");
    const PgPacked P = pg_pack(pin, off, n_graphs, node_off, edge_off, poses_w7, fixed, edges);
    const int *inc_off = P.inc_off; const unsigned char *fx = P.fx;

    /* ---- enqueue */
    PG_HIP(hipSetDevice(pg->ctx->device));
    hipStream_t st = pg->ctx->stream;
    PG_HIP(hipMemcpyAsync(pg->d_in, pin, off[8], hipMemcpyHostToDevice, st));
    PgArgs<Edge> A;
    const size_t Nn = (size_t)N, En = (size_t)E;
    pg_device_views(pg, off, Nn, En, A);
    A.out_nodes = (double *)pg->d_out;
    A.rec = (ll_pg_record *)(pg->d_out + Nn * per_node * sizeof(double)); A.out_cost = (double *)A.rec;
    A.o = o; A.solve = solve ? 1 : 0;
    A.cD = A.cWL = A.cWR = A.cC = A.cr = nullptr; A.cstat = nullptr;
    if (chain) {
        const PgChainWs cw = pg_chain_ws(pg);
        A.cD = cw.D; A.cWL = cw.WL; A.cWR = cw.WR; A.cC = cw.C; A.cr = cw.r; A.cstat = cw.stat;
    }
    PG_HIP(hipEventRecord(pg->ev[0], st));
    if (chain) hipLaunchKernelGGL((k_pg_solve<Edge, LL_PG_PRECOND_CHAIN>), dim3((unsigned)n_graphs), dim3(PG_THREADS), 0, st, A);
    else hipLaunchKernelGGL((k_pg_solve<Edge, LL_PG_PRECOND_BLOCK_JACOBI>), dim3((unsigned)n_graphs), dim3(PG_THREADS), 0, st, A);
    PG_HIP(hipEventRecord(pg->ev[1], st));
    PG_HIP(hipGetLastError());
    unsigned char *pout = pin + off[8];
    PG_HIP(hipMemcpyAsync(pout, pg->d_out, down, hipMemcpyDeviceToHost, st));
    const int *pstat = (const int *)(pout + pg_up8(down));
    if (chain) PG_HIP(hipMemcpyAsync((void *)pstat, A.cstat, stat_bytes, hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));                              /* the ONE synchronisation */
    pg->ms[solve ? 1 : 0] = ll_event_ms(pg->ev[0], pg->ev[1], pg->ms[solve ? 1 : 0]);

    /* ---- hand back */
    const double *nodes = (const double *)pout;
    const unsigned char *tail = pout + Nn * per_node * sizeof(double);
    if (!solve) {
        std::memcpy(out_b, nodes, Nn * 6 * sizeof(double));
        std::memcpy(out_a, tail, (size_t)n_graphs * sizeof(double));
        return LL_OK;
    }
    const ll_pg_record *recs = (const ll_pg_record *)tail;
    double *poses_out = out_a;
    for (int g = 0; g < n_graphs; ++g) {
        pg->counts[1] += recs[g].lm_iterations; pg->counts[2] += recs[g].pcg_iterations;
        if (chain) { pg->pc_counts[0] += pstat[2 * g]; pg->pc_counts[1] += pstat[2 * g + 1]; }
        if (recs[g].lm_successes == 0) continue;                  /* nothing accepted: the input comes back bit for bit */
        for (int k = node_off[g]; k < node_off[g + 1]; ++k)       /* so do fixed nodes and nodes without an edge */
            if (!fx[k] && inc_off[k + 1] > inc_off[k]) std::memcpy(poses_out + (size_t)k * 7, nodes + (size_t)k * 7, 7 * sizeof(double));
    }
    if (out_b) std::memcpy(out_b, recs, (size_t)n_graphs * sizeof(ll_pg_record));
    return LL_OK;
}

extern "C" int ll_posegraphs_evaluate(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                                      const unsigned char *fixed, const ll_pg_edge *edges, double *cost, double *grad6)
{
    return pg_run(pg, false, n_graphs, node_off, edge_off, poses_w7, fixed, edges, nullptr, cost, grad6);
}

extern "C" int ll_posegraphs_solve(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, double *poses_w7,
                                   const unsigned char *fixed, const ll_pg_edge *edges, const ll_pg_options *opt, ll_pg_record *rec)
{
    return pg_run(pg, true, n_graphs, node_off, edge_off, poses_w7, fixed, edges, opt, poses_w7, rec);
}

/* ll_pose_info -> the square-root information of the edge it stands for (the contract and the derivation are in the header):
 * Lambda = M^-T H M^-1 / sigma^2 + floor I with M^-1 = blkdiag(R(X) / 2, R(X)), then its upper Cholesky factor.  Host arithmetic only. */
extern "C" int ll_pg_edge_from_info(const ll_pose_info *info, const double *X_w7, double sigma, double floor, double S36[36])
{
    if (!info || !X_w7 || !S36) return LL_ERR_ARG;
    if (!ll_finite_n(X_w7, 7) || !std::isfinite(sigma) || !std::isfinite(floor) || floor < 0.0 || ll_zero_quat(X_w7)) return LL_ERR_ARG;
    if (info->flags & 1) return LL_ERR_STATE;
    double s2 = sigma * sigma;
    if (!(sigma > 0.0)) {
        if (!(info->sigma2 > 0.0) || !std::isfinite(info->sigma2)) return LL_ERR_STATE;
        s2 = info->sigma2;
    }
    double qx[4], R[3][3], Mi[6][6] = {}, HM[6][6], L[6][6];
    ll_quat_unit(X_w7, qx);
    ll_quat_matrix(qx, R);
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) { Mi[a][b] = 0.5 * R[a][b]; Mi[3 + a][3 + b] = R[a][b]; }
    for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) { double s = 0.0; for (int k = 0; k < 6; ++k) s += info->H[a * 6 + k] * Mi[k][b]; HM[a][b] = s; }
    for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) { double s = 0.0; for (int k = 0; k < 6; ++k) s += Mi[k][a] * HM[k][b]; L[a][b] = s / s2; }
    for (int a = 0; a < 6; ++a) for (int b = a + 1; b < 6; ++b) { const double m = 0.5 * (L[a][b] + L[b][a]); L[a][b] = m; L[b][a] = m; }
    for (int a = 0; a < 6; ++a) L[a][a] += floor;
    double U[6][6] = {};                                           /* U^T U = Lambda, row by row */
    for (int a = 0; a < 6; ++a) {
        double d = L[a][a];
        for (int k = 0; k < a; ++k) d -= U[k][a] * U[k][a];
        if (!(d > 0.0) || !std::isfinite(d)) return LL_ERR_STATE;
        U[a][a] = std::sqrt(d);
        for (int b = a + 1; b < 6; ++b) {
            double s = L[a][b];
            for (int k = 0; k < a; ++k) s -= U[k][a] * U[k][b];
            U[a][b] = s / U[a][a];
        }
    }
    for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) { if (!std::isfinite(U[a][b])) return LL_ERR_STATE; }
    for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) S36[a * 6 + b] = U[a][b];
    return LL_OK;
}

extern "C" int ll_posegraphs_evaluate6(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                                       const unsigned char *fixed, const ll_pg_edge6 *edges, double *cost, double *grad6)
{
    return pg_run(pg, false, n_graphs, node_off, edge_off, poses_w7, fixed, edges, nullptr, cost, grad6);
}

extern "C" int ll_posegraphs_solve6(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, double *poses_w7,
                                    const unsigned char *fixed, const ll_pg_edge6 *edges, const ll_pg_options *opt, ll_pg_record *rec)
{
    return pg_run(pg, true, n_graphs, node_off, edge_off, poses_w7, fixed, edges, opt, poses_w7, rec);
}

/* ms2: device time of the last evaluate and of the last solve; counts3: graphs of the last call, LM and PCG iterations of the last solve */
extern "C" int ll_posegraphs_timing(ll_posegraphs *pg, double *ms2, long long *counts3)
{
    if (!pg) return LL_ERR_ARG;
    if (ms2) for (int k = 0; k < 2; ++k) ms2[k] = pg->ms[k];
    if (counts3) for (int k = 0; k < 3; ++k) counts3[k] = pg->counts[k];
    return LL_OK;
}

/* the chain preconditioner's solver alone: n_systems block-tridiagonal systems, one workgroup each, the device functions k_pg_solve
 * uses.  Validates, packs into page-locked scratch, uploads into the workspace, launches, downloads, synchronises ONCE. */
extern "C" int ll_posegraphs_chain_solve(ll_posegraphs *pg, int n_systems, const int *node_off, const double *diag36, const double *upper36,
                                         const double *rhs6, double *out6, int *status)
{
    if (!pg) return LL_ERR_ARG;
    auto bad = [&](int code, const std::string &what) { return pg_fail(pg, code, "chain_solve: " + what); };
    if (n_systems < 0 || !node_off) return bad(LL_ERR_ARG, "n_systems < 0, or node_off is NULL");
    if (n_systems > pg->max_graphs) return bad(LL_ERR_CAPACITY, std::to_string(n_systems) + " systems exceed max_graphs " + std::to_string(pg->max_graphs));
    if (node_off[0] != 0) return bad(LL_ERR_ARG, "offsets must start at 0");
    for (int g = 0; g < n_systems; ++g)
        if (node_off[g + 1] < node_off[g]) return bad(LL_ERR_ARG, "system " + std::to_string(g) + ": offsets do not ascend");
    const int N = node_off[n_systems];
    if (N > pg->max_nodes) return bad(LL_ERR_CAPACITY, std::to_string(N) + " nodes exceed max_nodes_total " + std::to_string(pg->max_nodes));
    if (n_systems > 0 && !status) return bad(LL_ERR_ARG, "status is NULL");
    if (N > 0 && (!diag36 || !upper36 || !rhs6 || !out6)) return bad(LL_ERR_ARG, "diag36, upper36, rhs6 or out6 is NULL");
    for (int g = 0; g < n_systems; ++g)
        for (int k = node_off[g]; k < node_off[g + 1]; ++k) {
            const bool last = k + 1 == node_off[g + 1];            /* its coupling is not read */
            if (!ll_finite_n(diag36 + (size_t)k * 36, 36) || (!last && !ll_finite_n(upper36 + (size_t)k * 36, 36)) || !ll_finite_n(rhs6 + (size_t)k * 6, 6))
                return bad(LL_ERR_ARG, "system " + std::to_string(g) + ", node " + std::to_string(k - node_off[g]) + ": a block or the right-hand side is not finite");
        }
    if (n_systems == 0) return LL_OK;
    { const int rc = pg_chain_alloc(pg); if (rc) return rc; }

    const size_t Nn = (size_t)N, b36 = Nn * 36 * sizeof(double), b6 = Nn * 6 * sizeof(double);
    const size_t boff = pg_up8((size_t)(n_systems + 1) * sizeof(int)), bstat = pg_up8((size_t)n_systems * sizeof(int));
    unsigned char *pin = (unsigned char *)ll_pinned_scratch(boff + 2 * b36 + 2 * b6 + bstat);
    if (!pin) return bad(LL_ERR_HIP, "no page-locked scratch");
    unsigned char *p_diag = pin + boff, *p_up = p_diag + b36, *p_rhs = p_up + b36, *p_out = p_rhs + b6, *p_stat = p_out + b6;
    std::memcpy(pin, node_off, (size_t)(n_systems + 1) * sizeof(int));
    if (N > 0) { std::memcpy(p_diag, diag36, b36); std::memcpy(p_up, upper36, b36); std::memcpy(p_rhs, rhs6, b6); }
    const PgChainWs cw = pg_chain_ws(pg);
    PG_HIP(hipSetDevice(pg->ctx->device));
    hipStream_t st = pg->ctx->stream;
    PG_HIP(hipMemcpyAsync(cw.node_off, pin, (size_t)(n_systems + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (N > 0) {
        PG_HIP(hipMemcpyAsync(cw.D, p_diag, b36, hipMemcpyHostToDevice, st));
        PG_HIP(hipMemcpyAsync(cw.C, p_up, b36, hipMemcpyHostToDevice, st));
        PG_HIP(hipMemcpyAsync(cw.r, p_rhs, b6, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_pg_chain_solve, dim3((unsigned)n_systems), dim3(PG_THREADS), 0, st, cw.node_off, cw.D, cw.WL, cw.WR, cw.C, cw.r, cw.z, cw.status);
    PG_HIP(hipGetLastError());
    if (N > 0) PG_HIP(hipMemcpyAsync(p_out, cw.z, b6, hipMemcpyDeviceToHost, st));
    PG_HIP(hipMemcpyAsync(p_stat, cw.status, (size_t)n_systems * sizeof(int), hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));                              /* the ONE synchronisation */
    if (N > 0) std::memcpy(out6, p_out, b6);
    std::memcpy(status, p_stat, (size_t)n_systems * sizeof(int));
    return LL_OK;
}

/* ------------------------------------------------------------------ covariances: host side */
extern "C" void ll_pg_cov_default_options(ll_pg_cov_options *o)
{
    if (!o) return;
    o->max_pcg_iterations = 1000; o->tolerance = 1e-10;
}

/* validate, deduplicate the sources, pack, upload, three launches, download, synchronise ONCE */
template <typename Edge>
static int pg_cov_run(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7, const unsigned char *fixed,
                      const Edge *edges, int n_queries, const ll_pg_cov_query *q, const ll_pg_cov_options *opt, double *joint144, ll_pg_cov_record *rec)
{
    if (!pg) return LL_ERR_ARG;
    const char *who = "covariances: ";
    auto bad = [&](int code, const std::string &what) { return pg_fail(pg, code, who + what); };
    { const int rc = pg_check_layout(pg, who, n_graphs, node_off, edge_off, poses_w7, edges); if (rc) return rc; }
    const int N = node_off[n_graphs], E = edge_off[n_graphs];
    if (n_queries < 0 || (n_queries > 0 && (!q || !joint144))) return bad(LL_ERR_ARG, "n_queries < 0, or queries / joint144 is NULL");
    ll_pg_cov_options co;
    ll_pg_cov_default_options(&co);
    if (opt) co = *opt;
    if (co.max_pcg_iterations < 1 || !std::isfinite(co.tolerance) || co.tolerance < 0.0)
        return bad(LL_ERR_ARG, "options out of range (max_pcg_iterations >= 1, tolerance >= 0 and finite)");
    { const int rc = pg_check_graphs(pg, who, n_graphs, node_off, edge_off, poses_w7, fixed, edges); if (rc) return rc; }
    auto is_fixed = [&](int g, int n) { return fixed ? fixed[node_off[g] + n] != 0 : n == 0; };
    for (int k = 0; k < n_queries; ++k) {
        const std::string qs = "query " + std::to_string(k);
        if (q[k].graph < 0 || q[k].graph >= n_graphs) return bad(LL_ERR_ARG, qs + ": graph " + std::to_string(q[k].graph) + " lies outside the call");
        const int n = node_off[q[k].graph + 1] - node_off[q[k].graph];
        if (q[k].a < 0 || q[k].a >= n) return bad(LL_ERR_ARG, qs + ": node " + std::to_string(q[k].a) + " lies outside graph " + std::to_string(q[k].graph));
        if (q[k].b >= n) return bad(LL_ERR_ARG, qs + ": node " + std::to_string(q[k].b) + " lies outside graph " + std::to_string(q[k].graph));
    }
    /* H is singular on a component without a fixed node: union-find over the edges of every queried graph */
    std::vector<int> qgraphs;
    for (int k = 0; k < n_queries; ++k) qgraphs.push_back(q[k].graph);
    std::sort(qgraphs.begin(), qgraphs.end());
    qgraphs.erase(std::unique(qgraphs.begin(), qgraphs.end()), qgraphs.end());
    std::vector<int> parent((size_t)N);
    std::vector<unsigned char> anchored((size_t)N, 0);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; };
    for (int g : qgraphs) {
        const int n0 = node_off[g];
        for (int e = edge_off[g]; e < edge_off[g + 1]; ++e) {
            const int a = find(n0 + edges[e].i), b = find(n0 + edges[e].j);
            if (a != b) parent[a > b ? a : b] = a > b ? b : a;
        }
        for (int n = n0; n < node_off[g + 1]; ++n) if (is_fixed(g, n - n0)) anchored[find(n)] = 1;
    }
    for (int k = 0; k < n_queries; ++k)
        for (int node : {q[k].a, q[k].b})
            if (node >= 0 && !anchored[find(node_off[q[k].graph] + node)])
                return bad(LL_ERR_ARG, "query " + std::to_string(k) + ": node " + std::to_string(node) + " of graph " + std::to_string(q[k].graph) +
                                       " is not connected to a fixed node through the edges (H is singular there)");
    pg->cov_counts[0] = n_queries; pg->cov_counts[1] = pg->cov_counts[2] = 0;
    pg->cov_ms[0] = pg->cov_ms[1] = 0.0;
    if (n_queries == 0) return LL_OK;

    /* ---- the sources: every free (graph, node) some query names, once, in ascending order */
    std::vector<std::pair<int, int>> keys;
    for (int k = 0; k < n_queries; ++k)
        for (int node : {q[k].a, q[k].b})
            if (node >= 0 && !is_fixed(q[k].graph, node)) keys.emplace_back(q[k].graph, node);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const size_t n_src = keys.size(), n_qg = qgraphs.size(), Q = (size_t)n_queries;
    auto source_of = [&](int g, int node) {
        if (node < 0 || is_fixed(g, node)) return -1;
        return (int)(std::lower_bound(keys.begin(), keys.end(), std::make_pair(g, node)) - keys.begin());
    };
    size_t total_rows = 0;                                         /* 36 doubles each */
    for (const auto &kq : keys) total_rows += 6 * (size_t)(node_off[kq.first + 1] - node_off[kq.first]);

    /* ---- the layout of d_cov: [graphs | sources | queries] uploaded, flags, [columns' records | joint | records] downloaded, rows */
    const size_t o_graphs = 0, o_src = o_graphs + pg_up8(n_qg * sizeof(int)), o_qry = o_src + n_src * sizeof(PgCovSource);
    const size_t up = o_qry + pg_up8(Q * sizeof(PgCovQuery));
    const size_t o_flags = up, o_col = o_flags + pg_up8((size_t)n_graphs * sizeof(int)), o_joint = o_col + n_src * 6 * sizeof(ll_pg_cov_record);
    const size_t o_rec = o_joint + Q * 144 * sizeof(double), o_rows = o_rec + Q * sizeof(ll_pg_cov_record);
    const size_t down = o_rows - o_col, need = o_rows + total_rows * 36 * sizeof(double);
    PG_HIP(hipSetDevice(pg->ctx->device));
    if (need > pg->cov_bytes) {
        if (pg->d_cov) (void)hipFree(pg->d_cov);
        pg->d_cov = nullptr; pg->cov_bytes = 0;
        if (hipMalloc((void **)&pg->d_cov, need) != hipSuccess) {
            (void)hipGetLastError();
            pg->d_cov = nullptr;
            return bad(LL_ERR_HIP, "the columns' workspace could not be allocated (" + std::to_string(need) + " bytes)");
        }
        pg->cov_bytes = need;
    }
    for (hipEvent_t &e : pg->cov_ev) if (!e) PG_HIP(hipEventCreate(&e));

    size_t off[9];
    pg_in_layout((size_t)n_graphs, (size_t)N, (size_t)E, sizeof(Edge), off);
    unsigned char *pin = (unsigned char *)ll_pinned_scratch(off[8] + up + down);
    if (!pin) return bad(LL_ERR_HIP, "no page-locked scratch");
    (void)pg_pack(pin, off, n_graphs, node_off, edge_off, poses_w7, fixed, edges);
    unsigned char *ptab = pin + off[8], *pout = ptab + up;
    std::memset(ptab, 0, up);
    std::memcpy(ptab + o_graphs, qgraphs.data(), n_qg * sizeof(int));
    PgCovSource *hs = (PgCovSource *)(ptab + o_src);
    long long row = 0;
    for (size_t s = 0; s < n_src; ++s) {
        const int n = node_off[keys[s].first + 1] - node_off[keys[s].first];
        hs[s].row = row; hs[s].graph = keys[s].first; hs[s].node = keys[s].second; hs[s].n = n; hs[s].pad = 0;
        row += 6LL * n;
    }
    PgCovQuery *hq = (PgCovQuery *)(ptab + o_qry);
    for (int k = 0; k < n_queries; ++k) {
        const bool pair = q[k].b >= 0 && q[k].b != q[k].a;
        hq[k].sa = source_of(q[k].graph, q[k].a); hq[k].sb = pair ? source_of(q[k].graph, q[k].b) : -1;
        hq[k].a = q[k].a; hq[k].b = pair ? q[k].b : -1;
    }

    /* ---- enqueue */
    const bool chain = pg->precond == LL_PG_PRECOND_CHAIN;         /* its workspace exists: set_preconditioner allocated it */
    hipStream_t st = pg->ctx->stream;
    PG_HIP(hipMemcpyAsync(pg->d_in, pin, off[8], hipMemcpyHostToDevice, st));
    PG_HIP(hipMemcpyAsync(pg->d_cov, ptab, up, hipMemcpyHostToDevice, st));
    PgArgs<Edge> A;
    pg_device_views(pg, off, (size_t)N, (size_t)E, A);
    A.out_nodes = nullptr; A.rec = nullptr; A.out_cost = nullptr; A.solve = 0;
    ll_pg_default_options(&A.o);
    A.cD = A.cWL = A.cWR = A.cC = A.cr = nullptr; A.cstat = nullptr;
    if (chain) {
        const PgChainWs cw = pg_chain_ws(pg);
        A.cD = cw.D; A.cWL = cw.WL; A.cWR = cw.WR; A.cC = cw.C; A.cr = cw.r; A.cstat = cw.stat;
    }
    const int *d_graphs = (const int *)(pg->d_cov + o_graphs);
    const PgCovSource *d_src = (const PgCovSource *)(pg->d_cov + o_src);
    const PgCovQuery *d_qry = (const PgCovQuery *)(pg->d_cov + o_qry);
    int *d_flags = (int *)(pg->d_cov + o_flags);
    ll_pg_cov_record *d_col = (ll_pg_cov_record *)(pg->d_cov + o_col), *d_rec = (ll_pg_cov_record *)(pg->d_cov + o_rec);
    double *d_joint = (double *)(pg->d_cov + o_joint), *d_rows = (double *)(pg->d_cov + o_rows);
    PG_HIP(hipEventRecord(pg->cov_ev[0], st));
    if (chain) hipLaunchKernelGGL((k_pg_cov_prepare<Edge, LL_PG_PRECOND_CHAIN>), dim3((unsigned)n_qg), dim3(PG_THREADS), 0, st, A, d_graphs, d_flags);
    else hipLaunchKernelGGL((k_pg_cov_prepare<Edge, LL_PG_PRECOND_BLOCK_JACOBI>), dim3((unsigned)n_qg), dim3(PG_THREADS), 0, st, A, d_graphs, d_flags);
    PG_HIP(hipEventRecord(pg->cov_ev[1], st));
    if (n_src > 0) {
        if (chain) hipLaunchKernelGGL((k_pg_cov_columns<Edge, LL_PG_PRECOND_CHAIN>), dim3((unsigned)(n_src * 6)), dim3(PG_THREADS), 0, st, A, d_src, d_flags,
                                      d_rows, d_col, co.max_pcg_iterations, co.tolerance);
        else hipLaunchKernelGGL((k_pg_cov_columns<Edge, LL_PG_PRECOND_BLOCK_JACOBI>), dim3((unsigned)(n_src * 6)), dim3(PG_THREADS), 0, st, A, d_src, d_flags,
                                d_rows, d_col, co.max_pcg_iterations, co.tolerance);
    }
    PG_HIP(hipEventRecord(pg->cov_ev[2], st));
    hipLaunchKernelGGL(k_pg_cov_gather, dim3((unsigned)Q), dim3(64), 0, st, d_qry, d_src, d_rows, d_col, d_joint, d_rec);
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(pout, pg->d_cov + o_col, down, hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));                              /* the ONE synchronisation */
    for (int k = 0; k < 2; ++k) pg->cov_ms[k] = ll_event_ms(pg->cov_ev[k], pg->cov_ev[k + 1], pg->cov_ms[k]);

    /* ---- hand back */
    const ll_pg_cov_record *cols = (const ll_pg_cov_record *)pout;
    pg->cov_counts[1] = (long long)n_src;
    for (size_t c = 0; c < n_src * 6; ++c) pg->cov_counts[2] += cols[c].pcg_iterations;
    std::memcpy(joint144, pout + (o_joint - o_col), Q * 144 * sizeof(double));
    if (rec) std::memcpy(rec, pout + (o_rec - o_col), Q * sizeof(ll_pg_cov_record));
    return LL_OK;
}

extern "C" int ll_posegraphs_covariances(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                                         const unsigned char *fixed, const ll_pg_edge *edges, int n_queries, const ll_pg_cov_query *q,
                                         const ll_pg_cov_options *opt, double *joint144, ll_pg_cov_record *rec)
{
    return pg_cov_run(pg, n_graphs, node_off, edge_off, poses_w7, fixed, edges, n_queries, q, opt, joint144, rec);
}

extern "C" int ll_posegraphs_covariances6(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7,
                                          const unsigned char *fixed, const ll_pg_edge6 *edges, int n_queries, const ll_pg_cov_query *q,
                                          const ll_pg_cov_options *opt, double *joint144, ll_pg_cov_record *rec)
{
    return pg_cov_run(pg, n_graphs, node_off, edge_off, poses_w7, fixed, edges, n_queries, q, opt, joint144, rec);
}

/* ms2: device time of the last call's prepare and of its columns; counts3: its queries, its sources, the PCG iterations of all its columns */
extern "C" int ll_posegraphs_cov_timing(ll_posegraphs *pg, double ms2[2], long long counts3[3])
{
    if (!pg) return LL_ERR_ARG;
    if (ms2) for (int k = 0; k < 2; ++k) ms2[k] = pg->cov_ms[k];
    if (counts3) for (int k = 0; k < 3; ++k) counts3[k] = pg->cov_counts[k];
    return LL_OK;
}

/* ------------------------------------------------------------------ the gate (host arithmetic only; the contract is in the header)
 * pg_error and pg_jacobians above, the text the solver linearises an edge with, at the normalised poses; R(q_z)^T t_z in the matrix form. */
/* L (lower, L L^T = M) of a symmetric 6 x 6; false at a pivot that is not positive and finite */
static bool pgh_chol6(const double M[6][6], double L[6][6])
{
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {
            double acc = M[i][j];
            for (int k = 0; k < j; ++k) acc -= L[i][k] * L[j][k];
            if (i == j) { if (!(acc > 0.0) || !std::isfinite(acc)) return false; L[i][i] = std::sqrt(acc); }
            else L[i][j] = acc / L[j][j];
        }
    return true;
}

extern "C" int ll_pg_edge_gate(const double *Pa_w7, const double *Pb_w7, const double *Z_w7, const double *S36, const double joint144[144],
                               double *chi2, double cov36[36])
{
    if (!Pa_w7 || !Pb_w7 || !Z_w7 || !joint144 || !chi2) return LL_ERR_ARG;
    if (!ll_finite_n(Pa_w7, 7) || !ll_finite_n(Pb_w7, 7) || !ll_finite_n(Z_w7, 7) || !ll_finite_n(joint144, 144) || (S36 && !ll_finite_n(S36, 36))) return LL_ERR_ARG;
    if (ll_zero_quat(Pa_w7) || ll_zero_quat(Pb_w7) || ll_zero_quat(Z_w7)) return LL_ERR_ARG;
    double Pa[7], Pb[7], Z[7], e[6], A[3][3], Ra[3][3], v[3], Ja[6][6], Jb[6][6], Cm[6][6], L[6][6];
    ll_pose_unit(Pa_w7, Pa); ll_pose_unit(Pb_w7, Pb); ll_pose_unit(Z_w7, Z);
    const double qzc[4] = {-Z[0], -Z[1], -Z[2], Z[3]};
    pg_error(Pa, Pb, qzc, Z + 4, true, e, A, Ra, v);
    pg_jacobians(A, Ra, v, Ja, Jb);
    for (int m = 0; m < 6; ++m)                                    /* C = J Sigma J^T, J = [J_a J_b] */
        for (int n = 0; n < 6; ++n) {
            double s = 0.0;
            for (int u = 0; u < 12; ++u) {
                double t = 0.0;
                for (int w = 0; w < 12; ++w) t += joint144[u * 12 + w] * (w < 6 ? Ja[n][w] : Jb[n][w - 6]);
                s += (u < 6 ? Ja[m][u] : Jb[m][u - 6]) * t;
            }
            Cm[m][n] = s;
        }
    if (S36) {                                                     /* + (S^T S)^-1 */
        double I[6][6], Li[6][6] = {};
        for (int m = 0; m < 6; ++m) for (int n = 0; n < 6; ++n) { double s = 0.0; for (int k = 0; k < 6; ++k) s += S36[k * 6 + m] * S36[k * 6 + n]; I[m][n] = s; }
        if (!pgh_chol6(I, L)) return LL_ERR_ARG;
        for (int c = 0; c < 6; ++c)                                /* L^-1, column by column */
            for (int i = c; i < 6; ++i) {
                double acc = i == c ? 1.0 : 0.0;
                for (int k = c; k < i; ++k) acc -= L[i][k] * Li[k][c];
                Li[i][c] = acc / L[i][i];
            }
        for (int m = 0; m < 6; ++m) for (int n = 0; n < 6; ++n) { double s = 0.0; for (int k = 0; k < 6; ++k) s += Li[k][m] * Li[k][n]; Cm[m][n] += s; }
    }
    for (int m = 0; m < 6; ++m) for (int n = m + 1; n < 6; ++n) { const double h = 0.5 * (Cm[m][n] + Cm[n][m]); Cm[m][n] = h; Cm[n][m] = h; }
    if (!pgh_chol6(Cm, L)) return LL_ERR_ARG;
    double y[6], c2 = 0.0;                                         /* chi2 = |L^-1 e|^2 */
    for (int i = 0; i < 6; ++i) {
        double acc = e[i];
        for (int k = 0; k < i; ++k) acc -= L[i][k] * y[k];
        y[i] = acc / L[i][i];
        c2 += y[i] * y[i];
    }
    if (!std::isfinite(c2)) return LL_ERR_ARG;
    *chi2 = c2;
    if (cov36) for (int m = 0; m < 6; ++m) for (int n = 0; n < 6; ++n) cov36[m * 6 + n] = Cm[m][n];
    return LL_OK;
}
