/*
 * ll_deskew.hip -- TransformToEnd (laserOdometry.cpp:99-114, DISTORTION 1): the less-sharp, less-flat and -- mode 2 -- full-resolution
 * clouds of a solved frame re-projected, in place, to the end of its sweep = the start of the next one.  The reference has the function
 * and calls it under `if (0)` (:861) because KITTI arrives deskewed; ll_set_deskew switches it on for the frame loops, ll_deskew_slots
 * runs it alone (ll_api.hip).
 *
 * Per point p = (x, y, z, intensity), with the frame's q_last_curr / t_last_curr as the solve left them (never normalised):
 *   s   = (intensity - int(intensity)) / 0.1                        ll_point_s (:81-82)
 *   un  = Identity.slerp(s, q) * p + s * t   f64, stored to f32     TransformToStart (:86-93): the expressions of k_associate, so its bits
 *   end = q.inverse() * ((double)un - t)     f64, stored to f32     (:105-110); Eigen 3.3 inverse() = conjugate / squaredNorm, the zero
 *                                                                   quaternion unless squaredNorm > 0; q * v = _transformVector (ll_rotate)
 *   intensity = int(intensity)                                      (:113)
 * What depends on the pose only -- theta = acos|q.w|, sin theta, slerp's linear branch, the inverse -- is computed by one thread per
 * workgroup; a point costs the two sines of slerp's scales.  ll_deskew_scales restates ll_slerp_identity (ll_factor_math.h) with those
 * hoisted: the same operations on the same operands in the same order, so the same bits (the library is built without contraction).
 *
 * One launch covers every cloud of every slot it is given.  Work item = (slot, row, 256-point block of the row); rows of a slot:
 *   0              the less-sharp cloud (contiguous, hdr.n_less_sharp)
 *   1 .. R         the less-flat cloud: ring r's row of ring_nlf[r] points at stride ring_cap (hdr.lf_strided), or -- a contiguous
 *                  cloud of hdr.n_less_flat points (ll_upload_features, a restored checkpoint) -- a grid-stride share of it
 *   R+1 .. 2R      mode 2: laserCloud, ring r's row of ring_off[r + 1] - ring_off[r] points at stride ring_cap (a slot without one,
 *                  hdr.n = 0, has nothing here)
 * A thread moves one float4 in and one out; consecutive threads take consecutive points of a row.  Nothing of a slot with
 * hdr.status != 0 is read or written; the row variant also skips the slots whose row_mode bit 0 is clear (k_associate_rows' rule).
 * The kernels take the context's view as it is and the pose array / mode as arguments of their own: LLView keeps its members.
 */
#include "ll_associate.h"

struct LLDeskewPose {
    double q[4], t[3];
    double qi[4];                  /* q.inverse() */
    double theta, sinT, sgn_neg;   /* acos|q.w|, sin theta; sgn_neg != 0: q.w < 0 (slerp flips scale1) */
    int linear;                    /* |q.w| >= 1 - eps: scale0 = 1 - s, scale1 = s */
};

/* the part of ll_slerp_identity that does not depend on s */
__device__ __forceinline__ void ll_deskew_pose_setup(const double *pose7, LLDeskewPose &P)
{
    for (int k = 0; k < 4; ++k) P.q[k] = pose7[k];
    for (int k = 0; k < 3; ++k) P.t[k] = pose7[4 + k];
    const double one = 1.0 - 2.220446049250313e-16;
    const double d = (0.0 * P.q[0] + 0.0 * P.q[1]) + (0.0 * P.q[2] + 1.0 * P.q[3]);
    const double absD = fabs(d);
    P.linear = absD >= one;
    P.theta = 0.0; P.sinT = 1.0;
    if (!P.linear) { P.theta = acos(absD); P.sinT = sin(P.theta); }
    P.sgn_neg = d < 0.0 ? 1.0 : 0.0;
    /* Eigen 3.3 QuaternionBase::inverse(): conjugate().coeffs() / squaredNorm(), Quaternion(0, 0, 0, 0) unless squaredNorm() > 0 */
    const double n2 = P.q[0] * P.q[0] + P.q[1] * P.q[1] + P.q[2] * P.q[2] + P.q[3] * P.q[3];
    if (n2 > 0.0) { P.qi[0] = -P.q[0] / n2; P.qi[1] = -P.q[1] / n2; P.qi[2] = -P.q[2] / n2; P.qi[3] = P.q[3] / n2; }
    else { P.qi[0] = P.qi[1] = P.qi[2] = P.qi[3] = 0.0; }
}

/* ... and the part that does: qs = Identity.slerp(s, q) */
__device__ __forceinline__ void ll_deskew_scales(const LLDeskewPose &P, double s, double qs[4])
{
    double scale0, scale1;
    if (P.linear) { scale0 = 1.0 - s; scale1 = s; }
    else {
        const double a0 = (1.0 - s) * P.theta, a1 = s * P.theta;
        scale0 = sin(a0) / P.sinT; scale1 = sin(a1) / P.sinT;
    }
    if (P.sgn_neg != 0.0) scale1 = -scale1;
    qs[0] = scale0 * 0.0 + scale1 * P.q[0]; qs[1] = scale0 * 0.0 + scale1 * P.q[1];
    qs[2] = scale0 * 0.0 + scale1 * P.q[2]; qs[3] = scale0 * 1.0 + scale1 * P.q[3];
}

__device__ __forceinline__ float4 ll_deskew_point(const LLDeskewPose &P, const float4 p)
{
    const double s = ll_point_s(1, p);
    const double v[3] = {(double)p.x, (double)p.y, (double)p.z};
    double qs[4], rr[3];
    ll_deskew_scales(P, s, qs);
    ll_rotate(qs, v, rr);
    const float ux = (float)(rr[0] + s * P.t[0]), uy = (float)(rr[1] + s * P.t[1]), uz = (float)(rr[2] + s * P.t[2]);   /* :89-93 */
    const double w[3] = {(double)ux - P.t[0], (double)uy - P.t[1], (double)uz - P.t[2]};
    double e[3];
    ll_rotate(P.qi, w, e);                                                                                                /* :105 */
    return make_float4((float)e[0], (float)e[1], (float)e[2], (float)(int)p.w);                                            /* :108-113 */
}

#define LL_DK_BLOCK 256
/* pose: [.][7], the pose of slot s at pose + (s - pose_base) * 7 (V.pose with pose_base 0, or the call's own uploaded array) */
template <bool ROWS>
__global__ __launch_bounds__(LL_DK_BLOCK) void k_deskew(LLView V, int first, int count, const double *pose, int pose_base, int mode, int nbx)
{
    const int R = V.R, rows = 1 + R + (mode == 2 ? R : 0);
    const int bx = blockIdx.x % nbx, row = (blockIdx.x / nbx) % rows, sl = blockIdx.x / (nbx * rows);
    if (sl >= count) return;
    const int s = first + sl;
    if (ROWS && (V.row_mode[s] & 1) == 0) return;             /* the sequence sits out: every byte of its slot stays */
    const ScanHdr h = V.hdr[s];
    if (h.status != 0) return;                                /* a refused scan: nothing read, nothing written */
    /* the block's points: n of them from base, this block's first at i0, the next share stride further on */
    float4 *base; int n, i0 = bx * LL_DK_BLOCK, stride = nbx * LL_DK_BLOCK;
    if (row == 0) {
        base = V.lsharp + (size_t)s * V.cap_lsharp; n = min(h.n_less_sharp, V.cap_lsharp);
    } else if (row <= R) {
        const int r = row - 1;
        if (h.lf_strided) { base = V.lflat + (size_t)s * V.LFS + (size_t)r * V.ring_cap; n = min(V.ring_nlf[(size_t)s * R + r], V.ring_cap); }
        else { base = V.lflat + (size_t)s * V.LFS; n = min(h.n_less_flat, V.LFS); i0 += r * stride; stride *= R; }
    } else {
        const int r = row - 1 - R;
        const int *ro = V.ring_off + (size_t)s * (R + 1);
        const int off = ro[r];
        base = V.cloud + (size_t)s * V.CS + (size_t)r * V.ring_cap;
        n = (h.n > 0 && off >= 0) ? min(ro[r + 1] - off, V.ring_cap) : 0;
    }
    if (i0 >= n) return;
    __shared__ LLDeskewPose P;
    if (threadIdx.x == 0) ll_deskew_pose_setup(pose + (size_t)(s - pose_base) * 7, P);
    __syncthreads();
    for (int i = i0 + (int)threadIdx.x; i < n; i += stride) base[i] = ll_deskew_point(P, base[i]);
}

/* rows != 0: the row variant (slots with row_mode bit 0 only).  0, or -1 when the range needs more workgroups than a launch holds */
int ll_launch_deskew(const LLView &V, int first, int count, const double *pose, int pose_base, int mode, int rows, hipStream_t st)
{
    if (count <= 0) return 0;
    const int longest = V.ring_cap > V.cap_lsharp ? V.ring_cap : V.cap_lsharp;
    const int nbx = (longest + LL_DK_BLOCK - 1) / LL_DK_BLOCK;
    const long long blocks = (long long)count * (1 + V.R + (mode == 2 ? V.R : 0)) * nbx;
    if (blocks > 0x7fffffffLL) return -1;                     /* more than one launch holds: the caller reports it */
    if (rows) hipLaunchKernelGGL(k_deskew<true>, dim3((unsigned)blocks), dim3(LL_DK_BLOCK), 0, st, V, first, count, pose, pose_base, mode, nbx);
    else hipLaunchKernelGGL(k_deskew<false>, dim3((unsigned)blocks), dim3(LL_DK_BLOCK), 0, st, V, first, count, pose, pose_base, mode, nbx);
    return 0;
}
