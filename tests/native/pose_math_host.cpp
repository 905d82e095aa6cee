// csrc/ll_pose_math.h on the host alone: the program includes nothing of the library but that header.
// stdin:  "N M", then N cases of 17 doubles (pose a, pose b, vector v) and M poses of 7, every double as 16 hex digits of its bits.
// stdout: per case one line with the bits of, in this order,
//           ll_qmul(a, b) 4, the same with the output on a 4, on b 4, ll_rotate(a, v) 3, ll_quat_matrix(a) 9, ll_mat_apply of it on v 3
//           and on v in place 3, ll_quat_unit(a) 4 and in place 4, ll_pose_unit(a) 7, ll_pose_compose(a, b) 7, onto a 7, onto b 7,
//           ll_pose_inverse(a) 7 and in place 7                                                                    = 80 words;
//         per pose one line "ll_finite_n(p, 7) ll_zero_quat(p)".
// Built with g++ -O2 -ffp-contract=off by tests/test_pose_math_host.py, which restates every operation and compares bit for bit.
#include "ll_pose_math.h"

#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

static bool read(double *p, int n)
{
    for (int k = 0; k < n; ++k) {
        uint64_t u;
        if (std::scanf("%" SCNx64, &u) != 1) return false;
        std::memcpy(p + k, &u, 8);
    }
    return true;
}

static void put(const double *p, int n)
{
    for (int k = 0; k < n; ++k) {
        uint64_t u;
        std::memcpy(&u, p + k, 8);
        std::printf("%016" PRIx64 " ", u);
    }
}

int main()
{
    int N, M;
    if (std::scanf("%d %d", &N, &M) != 2) return 2;
    for (int c = 0; c < N; ++c) {
        double a[7], b[7], v[3], o[9], R[3][3];
        if (!read(a, 7) || !read(b, 7) || !read(v, 3)) return 2;
        ll_qmul(a, b, o); put(o, 4);
        std::memcpy(o, a, 32); ll_qmul(o, b, o); put(o, 4);
        std::memcpy(o, b, 32); ll_qmul(a, o, o); put(o, 4);
        ll_rotate(a, v, o); put(o, 3);
        ll_quat_matrix(a, R); put(&R[0][0], 9);
        ll_mat_apply(R, v, o); put(o, 3);
        std::memcpy(o, v, 24); ll_mat_apply(R, o, o); put(o, 3);
        ll_quat_unit(a, o); put(o, 4);
        std::memcpy(o, a, 32); ll_quat_unit(o, o); put(o, 4);
        ll_pose_unit(a, o); put(o, 7);
        ll_pose_compose(a, b, o); put(o, 7);
        std::memcpy(o, a, 56); ll_pose_compose(o, b, o); put(o, 7);
        std::memcpy(o, b, 56); ll_pose_compose(a, o, o); put(o, 7);
        ll_pose_inverse(a, o); put(o, 7);
        std::memcpy(o, a, 56); ll_pose_inverse(o, o); put(o, 7);
        std::printf("\n");
    }
    for (int c = 0; c < M; ++c) {
        double p[7];
        if (!read(p, 7)) return 2;
        std::printf("%d %d\n", ll_finite_n(p, 7) ? 1 : 0, ll_zero_quat(p) ? 1 : 0);
    }
    return 0;
}
