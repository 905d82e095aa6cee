/* ll_cubemap_tables.h -- the host-side bookkeeping of a cube map, once: the (offset, count) pair tables, the centre cube, the shift
 * loops and the valid cubes (laserMapping.cpp:1584-1801) and the update of :2103-2165 as plan -> fit -> commit.  Plain host C++
 * without a device pointer: ll_cubemap.hip, ll_cubemaps.hip and ll_map_merge.hip turn the pieces handed out here into their own
 * copy descriptors, launch them, and keep their own `broken` handling around the commit. */
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#define CM_W 21
#define CM_H 21
#define CM_D 11
#define CM_N (CM_W * CM_H * CM_D)     /* 4851 (:53) */

/* the layout of one map: cube c of type w (0 corner, 1 surf) is cnt[w][c] points from off[w][c] on in pool cur[w] of the type, which
 * is filled up to top[w] of cap_pool points.  cen: the array index of the world's origin cube; valid: the last prepare's cubes */
struct CmTables {
    int cen[3] = {10, 10, 5};
    size_t cap_pool = 0, top[2] = {0, 0};
    int cur[2] = {0, 0};
    std::vector<int> off[2] = {std::vector<int>(CM_N, 0), std::vector<int>(CM_N, 0)}, cnt[2] = {std::vector<int>(CM_N, 0), std::vector<int>(CM_N, 0)};
    int valid[125]; int n_valid = 0;
};

/* one step of a shift loop (:1598-1778): every cube takes the pair of its neighbour at -dir along the axis, the layer that has none
 * becomes empty.  One walk over the array against the move, so that a pair is read before it is overwritten */
inline void cm_shift(CmTables *cm, int axis, int dir)
{
    const int dim[3] = {CM_W, CM_H, CM_D}, stride[3] = {1, CM_W, CM_W * CM_H};
    for (int w = 0; w < 2; ++w)
        for (int n = 0; n < CM_N; ++n) {
            const int c = dir > 0 ? CM_N - 1 - n : n, from = c / stride[axis] % dim[axis] - dir;
            const bool in = from >= 0 && from < dim[axis];
            cm->off[w][c] = in ? cm->off[w][c - dir * stride[axis]] : 0;
            cm->cnt[w][c] = in ? cm->cnt[w][c - dir * stride[axis]] : 0;
        }
}

/* the cube the translation t_w3 falls into, in the indices the map has now: truncated (:1584-1586), one less below zero (:1588-1593) */
inline void cm_centre(const CmTables &cm, const double *t_w3, int cc[3])
{
    for (int k = 0; k < 3; ++k) cc[k] = (int)((t_w3[k] + 25.0) / 50.0) + cm.cen[k] - (t_w3[k] + 25.0 < 0 ? 1 : 0);
}

/* the cubes around cc that lie inside the array, in laserMapping's loop order (:1783-1801) -> their number (<= 125) */
inline int cm_valid_cubes(const int cc[3], int *valid)
{
    int n = 0;
    for (int i = cc[0] - 2; i <= cc[0] + 2; i++) for (int j = cc[1] - 2; j <= cc[1] + 2; j++) for (int k = cc[2] - 1; k <= cc[2] + 1; k++)
        if (i >= 0 && i < CM_W && j >= 0 && j < CM_H && k >= 0 && k < CM_D) valid[n++] = i + CM_W * j + CM_W * CM_H * k;
    return n;
}

/* prepare's table half: the array follows the centre cube of t_w3 until it lies 3 cubes inside on every axis, then the valid cubes */
inline void cm_follow(CmTables &cm, const double *t_w3)
{
    const int dim[3] = {CM_W, CM_H, CM_D};
    int cc[3]; cm_centre(cm, t_w3, cc);
    for (int k = 0; k < 3; ++k) {
        while (cc[k] < 3) { cm_shift(&cm, k, +1); cc[k]++; cm.cen[k]++; }          /* :1595-1625 and the J, K twins */
        while (cc[k] >= dim[k] - 3) { cm_shift(&cm, k, -1); cc[k]--; cm.cen[k]--; }
    }
    cm.n_valid = cm_valid_cubes(cc, cm.valid);
}

/* one copy a caller has to make for a cube: old_cnt points from old_off of the type's pool to dst, then new_cnt of the update's new
 * points, from new_first on in their by-cube sorted order, behind them.  Either count may be 0 */
struct CmPiece { int cube, old_off, old_cnt, new_first, new_cnt, dst; };

/* the update of one map and one cloud type (:2103-2165).  set [n_set]: the cubes that are voxel-filtered, one segment each in this
 * order -- a frame's valid cubes (empty segments included), or for a merge the cubes with new points, ascending.  addcnt [CM_N]: the
 * new points per cube.  goff [CM_N + 1]: where a cube's new points begin in the by-cube order; seg_off [n_set + 1] and pieces: the
 * filter input, a cube's cloud followed by its new points (:2119-2125); grown: the cubes outside the set that received points,
 * ascending -- none in most frames and in every merge, which the counts show without a walk over the array */
struct CmPlan { std::vector<int> goff, seg_off, grown; std::vector<CmPiece> pieces; };

inline CmPlan cm_plan(const CmTables &cm, int w, const int *set, int n_set, const int *addcnt)
{
    CmPlan p;
    p.goff.assign(CM_N + 1, 0); p.seg_off.reserve(n_set + 1); p.seg_off.push_back(0); p.pieces.reserve(n_set);
    for (int c = 0; c < CM_N; ++c) p.goff[c + 1] = p.goff[c] + addcnt[c];
    int outside = p.goff[CM_N];
    for (int v = 0; v < n_set; ++v) {
        const int c = set[v], at = p.seg_off.back(), old = cm.cnt[w][c];
        if (old > 0 || addcnt[c] > 0) p.pieces.push_back({c, cm.off[w][c], old, p.goff[c], addcnt[c], at});
        p.seg_off.push_back(at + old + addcnt[c]);
        outside -= addcnt[c];
    }
    if (outside > 0) {
        std::vector<char> in(CM_N, 0);
        for (int v = 0; v < n_set; ++v) in[set[v]] = 1;
        for (int c = 0; c < CM_N; ++c) if (!in[c] && addcnt[c] > 0) p.grown.push_back(c);
    }
    return p;
}

/* the longest segment of an offset table (what ll_voxel_grid_segments wants to know) */
inline int cm_max_segment(const std::vector<int> &o) { int m = 0; for (size_t s = 1; s < o.size(); ++s) m = std::max(m, o[s] - o[s - 1]); return m; }

/* Will it fit, once the filter has left seg_count [n_set] points of the set's cubes?  need: those + the grown clouds, old + new.  A
 * pool that would be 3/4 full is compacted by the commit, and a compaction keeps the clouds outside the set only: these + need must
 * fit.  false: *err says so.  Nothing is changed either way */
inline bool cm_fit(const CmTables &cm, int w, const CmPlan &p, const int *set, int n_set, const int *addcnt, const int *seg_count, size_t *need, std::string *err)
{
    size_t nd = 0, live = 0;
    for (int v = 0; v < n_set; ++v) nd += (size_t)seg_count[v];
    for (const int c : p.grown) nd += (size_t)cm.cnt[w][c] + (size_t)addcnt[c];
    *need = nd;
    if (cm.top[w] + nd <= cm.cap_pool * 3 / 4) return true;
    for (int c = 0; c < CM_N; ++c) live += (size_t)cm.cnt[w][c];
    for (int v = 0; v < n_set; ++v) live -= (size_t)cm.cnt[w][set[v]];
    if (live + nd > cm.cap_pool) { *err = "cube map pool exhausted (pool_points too small)"; return false; }
    return true;
}

/* the tables after the update (need: cm_fit's, or the filtered size where nothing grows), which cannot fail after a cm_fit that
 * said yes.  It leaves to its caller, in this order on the stream: moves -- a compaction's copies out of the pool that WAS current
 * into the one that is now; the filtered points, back to back in set order, to `at` of the current pool; grow -- per grown cube
 * its old cloud and the new points, within the current pool.  The set's old clouds are not carried through the compaction */
struct CmCommit { std::vector<CmPiece> moves, grow; size_t at = 0; };
inline CmCommit cm_commit(CmTables &cm, int w, const CmPlan &p, const int *set, int n_set, const int *addcnt, const int *seg_count, size_t need)
{
    CmCommit k;
    std::vector<int> &off = cm.off[w], &cnt = cm.cnt[w];
    for (int v = 0; v < n_set; ++v) cnt[set[v]] = 0;
    if (cm.top[w] + need > cm.cap_pool * 3 / 4) {                                  /* live clouds -> the other pool, back to back */
        size_t top = 0;
        for (int c = 0; c < CM_N; ++c)
            if (cnt[c] > 0) { k.moves.push_back({c, off[c], cnt[c], 0, 0, (int)top}); off[c] = (int)top; top += (size_t)cnt[c]; }
        cm.cur[w] ^= 1; cm.top[w] = top;
    }
    size_t at = k.at = cm.top[w];
    for (int v = 0; v < n_set; ++v) { off[set[v]] = (int)at; cnt[set[v]] = seg_count[v]; at += (size_t)seg_count[v]; }
    for (const int c : p.grown) {
        k.grow.push_back({c, off[c], cnt[c], p.goff[c], addcnt[c], (int)at});
        off[c] = (int)at; cnt[c] += addcnt[c]; at += (size_t)cnt[c];
    }
    cm.top[w] = at;
    return k;
}
