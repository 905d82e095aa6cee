/* ll_tiles.h -- the vocabulary of the tiled kernels, once: map export / import, checkpoints, map merge, keyframe insert, map
 * alignment, visibility and BEV all deal their work the same way.  The host knows every size, lists the work as a table of segments
 * -- each with its point count `cnt` and `tile0`, the tiles of the segments before it --, and launches one workgroup per fixed-size
 * tile; the workgroup finds its segment by a binary search over tile0 (the table is uniform per workgroup: scalar loads).
 *   LLTiler        numbers the tiles while the host builds a table, and says whether one launch can hold them;
 *   ll_tile_find   the search, for the kernels and (plainly compared) for the host;
 *   ll_copy_tile   the copy of one tile, every load before the first store (device only).
 * Plain C++ outside the __HIPCC__ parts: tests/native/tiles_host.cpp includes nothing but this header. */
#pragma once

#ifndef LL_HD
#if defined(__HIPCC__)
#define LL_HD __host__ __device__ __forceinline__
#else
#define LL_HD static inline
#endif
#endif

/* can one launch have n workgroups, and a 32-bit tile0 number them? */
LL_HD bool ll_grid_fits(unsigned long long n) { return n <= 0x7fffffffull; }

/* tile0 of a segment while a table is built. per: points per tile; next: the tiles handed out so far, the launch's grid size */
struct LLTiler {
    int per;
    unsigned long long next = 0;
    unsigned take(int cnt)                        /* the segment's tile0; a segment of cnt points takes ceil(cnt / per) tiles */
    {
        const unsigned tile0 = (unsigned)next;
        next += (unsigned long long)((cnt + per - 1) / per);
        return tile0;
    }
    bool fits() const { return ll_grid_fits(next); }      /* one launch holds the tiles, and every tile0 was exact */
};

/* the segment of tile t -- the last one whose first tile is <= t -- in a table of nseg >= 1 segments with a `tile0` member.  On the
 * device tile0 is read as what it is, the same for the whole wave */
template <typename S>
LL_HD int ll_tile_find(const S *seg, int nseg, unsigned t)
{
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
#if defined(__HIP_DEVICE_COMPILE__)
        if ((unsigned)__builtin_amdgcn_readfirstlane((int)seg[mid].tile0) <= t) lo = mid; else hi = mid;
#else
        if (seg[mid].tile0 <= t) lo = mid; else hi = mid;
#endif
    }
    return lo;
}

#if defined(__HIPCC__)
/* a pointer that comes out of a table: said to be global, not flat */
typedef float ll_f4 __attribute__((ext_vector_type(4)));
typedef ll_f4 __attribute__((address_space(1))) ll_gf4;

/* point K * 256 + tid of a tile of n >= 1 points, 256 lanes x U points: the loads of all U points are issued before the first store
 * (a clamped index instead of a branch between them; the recursion keeps the U values in registers) */
template <int U, int K>
__device__ __forceinline__ void ll_copy_tile(const ll_gf4 *src, ll_gf4 *out, int n, int tid)
{
    const int i = K * 256 + tid;
    const ll_f4 v = src[min(i, n - 1)];
    if constexpr (K + 1 < U) ll_copy_tile<U, K + 1>(src, out, n, tid);
    if (i < n) out[i] = v;
}
#endif
