/* ll_pose_math.h -- quaternion and pose-on-pose arithmetic, once (a pose acting on a POINT is ll_map_to_world, ll_map_search.h).
 * f64, a quaternion is (x, y, z, w), a pose is pose_w7 (qx, qy, qz, qw, tx, ty, tz).  Only + - * / and sqrt, every operation
 * rounded on its own (the build has -ffp-contract=off for host and device), so the kernels, the host entry points and
 * tests/native/pose_math_host.cpp -- which includes nothing but this header -- compute the same bits.
 * A rotation has TWO forms here, and they round differently; a caller keeps the one it has:
 *   Eigen form   ll_rotate, and on it ll_pose_compose / ll_pose_inverse: lightloam::WorldPose::compose and LaserMapping::qmul / qrot
 *                of the host chain.  Drives, BEV, deskew, the odometry association, the t_z term of the pose-graph error.
 *   matrix form  ll_quat_matrix, then ll_mat_apply row by row as (R0 v0 + R1 v1) + R2 v2.  PCM (ll_pcm_math.h builds its own
 *                compose / inverse on it), the translation error of the pose-graph edge, ll_pg_edge_gate, ll_pg_edge_from_info.
 * Plain C++ outside __HIPCC__. */
#pragma once
#include <math.h>

#ifndef LL_HD
#if defined(__HIPCC__)
#define LL_HD __host__ __device__ __forceinline__
#else
#define LL_HD static inline
#endif
#endif

/* o = a (x) b, the Hamilton product (LaserMapping::qmul).  All four components are formed before the first store: o may be a or b */
LL_HD void ll_qmul(const double *a, const double *b, double *o)
{
    const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    const double y = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    const double z = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}

/* out = q * v, Eigen's _transformVector: uv = u x v; uv += uv; v + w*uv + u x uv (LaserMapping::qrot on the host) */
LL_HD void ll_rotate(const double q[4], const double v[3], double out[3])
{
    const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
    double uvx = uy * v[2] - uz * v[1], uvy = uz * v[0] - ux * v[2], uvz = ux * v[1] - uy * v[0];
    uvx += uvx; uvy += uvy; uvz += uvz;
    out[0] = (v[0] + w * uvx) + (uy * uvz - uz * uvy);
    out[1] = (v[1] + w * uvy) + (uz * uvx - ux * uvz);
    out[2] = (v[2] + w * uvz) + (ux * uvy - uy * uvx);
}

/* R(q) of a unit quaternion, entry by entry */
LL_HD void ll_quat_matrix(const double *q, double (*R)[3])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z); R[0][1] = 2.0 * (x * y - z * w); R[0][2] = 2.0 * (x * z + y * w);
    R[1][0] = 2.0 * (x * y + z * w); R[1][1] = 1.0 - 2.0 * (x * x + z * z); R[1][2] = 2.0 * (y * z - x * w);
    R[2][0] = 2.0 * (x * z - y * w); R[2][1] = 2.0 * (y * z + x * w); R[2][2] = 1.0 - 2.0 * (x * x + y * y);
}

/* o = R v, every row as (R0 v0 + R1 v1) + R2 v2; o may be v */
LL_HD void ll_mat_apply(const double (*R)[3], const double *v, double *o)
{
    const double v0 = v[0], v1 = v[1], v2 = v[2];
    for (int k = 0; k < 3; ++k) o[k] = (R[k][0] * v0 + R[k][1] * v1) + R[k][2] * v2;
}

/* q / |q| with |q| = sqrt((xx + yy) + (zz + ww)); o may be q */
LL_HD void ll_quat_unit(const double *q, double *o)
{
    const double n = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    for (int k = 0; k < 4; ++k) o[k] = q[k] / n;
}

/* the pose with its quaternion normalised, the translation copied */
LL_HD void ll_pose_unit(const double *p, double *o)
{
    ll_quat_unit(p, o);
    for (int k = 4; k < 7; ++k) o[k] = p[k];
}

/* a o b = (q_a (x) q_b, R(q_a) t_b + t_a) in the Eigen form (transformAssociateToMap spells it so); o may be a or b */
LL_HD void ll_pose_compose(const double *a, const double *b, double *o)
{
    double r[3];
    ll_rotate(a, b + 4, r);
    for (int k = 0; k < 3; ++k) r[k] += a[4 + k];
    ll_qmul(a, b, o);
    for (int k = 0; k < 3; ++k) o[4 + k] = r[k];
}

/* inv(a) = (q_a*, -(R(q_a*) t_a)) of a pose with a unit quaternion, in the Eigen form; o may be a */
LL_HD void ll_pose_inverse(const double *a, double *o)
{
    const double c[4] = {-a[0], -a[1], -a[2], a[3]};
    double r[3];
    ll_rotate(c, a + 4, r);
    for (int k = 0; k < 4; ++k) o[k] = c[k];
    for (int k = 0; k < 3; ++k) o[4 + k] = -r[k];
}

/* what the host entry points ask of a pose before they compute with it.  x - x is 0 for a finite x and NaN otherwise: std::isfinite
 * without <cmath>, good only because the build has -fno-fast-math (tests/test_pose_math_host.py checks NaN, both infinities, the
 * largest double and a denormal) */
LL_HD bool ll_finite_n(const double *p, int n) { for (int k = 0; k < n; ++k) if (!(p[k] - p[k] == 0.0)) return false; return true; }
LL_HD bool ll_zero_quat(const double *q) { return q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0; }
