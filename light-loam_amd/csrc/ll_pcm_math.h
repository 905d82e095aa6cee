/* ll_pcm_math.h -- the pair arithmetic of ll_pcm (include/lightloam_hip.h states it float by float), once: k_pcm_prepare and
 * k_pcm_adjacency (ll_pcm.hip) and ll_pcm_host run this text, so the CPU tests of ll_pcm_host pin the device's arithmetic.  Only
 * + - * and comparisons in f64, every operation rounded on its own (the build has -ffp-contract=off for host and device).
 * A pose is pose_w7 (qx, qy, qz, qw, tx, ty, tz) with a unit quaternion: the host normalised it.  The product and the matrix are
 * ll_pose_math.h's; compose and inverse here are the MATRIX-form pair (ll_pose_compose / ll_pose_inverse round differently). */
#pragma once
#include "ll_pose_math.h"

#define PCM_HD __host__ __device__ __forceinline__
#define PCM_PREP 23                      /* per candidate: B 7, Ai 7, P_i 7, s_i, s_j */
#define PCM_MAX_C 4096                   /* one wave holds a row: 64 lanes of 64 bits */

struct PcmTol { double rot_tol, trans_tol, rot_rate, trans_rate; };

/* o = R(q) v in the matrix form: the matrix entry by entry, then every row as (R0 v0 + R1 v1) + R2 v2 */
PCM_HD void pcm_rotate(const double *q, const double *v, double *o)
{
    double R[3][3];
    ll_quat_matrix(q, R);
    ll_mat_apply(R, v, o);
}

/* a o b = (q_a (x) q_b, R(q_a) t_b + t_a) */
PCM_HD void pcm_compose(const double *a, const double *b, double *o)
{
    double r[3];
    ll_qmul(a, b, o);
    pcm_rotate(a, b + 4, r);
    o[4] = r[0] + a[4]; o[5] = r[1] + a[5]; o[6] = r[2] + a[6];
}

/* inv(a) = (q_a*, -(R(q_a*) t_a)) */
PCM_HD void pcm_inverse(const double *a, double *o)
{
    double r[3];
    o[0] = -a[0]; o[1] = -a[1]; o[2] = -a[2]; o[3] = a[3];
    pcm_rotate(o, a + 4, r);
    o[4] = -r[0]; o[5] = -r[1]; o[6] = -r[2];
}

/* what a pair needs of candidate (i, j, Z): B = Z o inv(P_j), Ai = (P_j o inv(Z)) o inv(P_i), P_i, s_i, s_j */
PCM_HD void pcm_prepare(const double *Pi, const double *Pj, const double *Z, double si, double sj, double *out)
{
    double inv[7], t[7];
    pcm_inverse(Pj, inv);
    pcm_compose(Z, inv, out);
    pcm_inverse(Z, inv);
    pcm_compose(Pj, inv, t);
    pcm_inverse(Pi, inv);
    pcm_compose(t, inv, out + 7);
    for (int k = 0; k < 7; ++k) out[14 + k] = Pi[k];
    out[21] = si; out[22] = sj;
}

/* the pair (c, d), c < d, from c's B, P_i, s_i, s_j and d's Ai, s_i, s_j */
PCM_HD bool pcm_pair(const double *Bc, const double *Pic, double sic, double sjc, const double *Aid, double sid, double sjd, const PcmTol &p)
{
    double T[7], E[7];
    pcm_compose(Bc, Aid, T);
    pcm_compose(T, Pic, E);
    const double rot2 = 4.0 * ((E[0] * E[0] + E[1] * E[1]) + E[2] * E[2]);
    const double trans2 = (E[4] * E[4] + E[5] * E[5]) + E[6] * E[6];
    const double di = sic - sid, dj = sjc - sjd;
    const double L = (di < 0.0 ? -di : di) + (dj < 0.0 ? -dj : dj);
    const double ar = p.rot_tol + p.rot_rate * L, at = p.trans_tol + p.trans_rate * L;
    const double ar2 = ar * ar, at2 = at * at;
    const bool finite = rot2 - rot2 == 0.0 && trans2 - trans2 == 0.0 && ar2 - ar2 == 0.0 && at2 - at2 == 0.0;
    return finite && rot2 <= ar2 && trans2 <= at2;
}
