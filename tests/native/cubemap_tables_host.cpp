// The cube map's pair-table bookkeeping (csrc/ll_cubemap_tables.h) against a naive model, on the host alone.
//
// The model is the reference's picture: one std::vector<int> of point ids per cube and cloud type, shifted row by row as the
// reference shuffles its cloud pointers, with a "voxel filter" that keeps every second id of a filtered cube.  A pool is an array
// of ids that the pieces handed out by the header are applied to, as the library's copy kernels would.  After every frame each
// cube's [off, off + cnt) must hold exactly the model's ids in order.  Built with -fsanitize=address,undefined by
// tests/test_cubemap_tables.py; exit status 0 = everything held.
#include "ll_cubemap_tables.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>

#define CHECK(cond, ...)                                                                     \
    do {                                                                                     \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } \
    } while (0)

static const int DIM[3] = {CM_W, CM_H, CM_D};
static int cube_at(int i, int j, int k) { return i + CM_W * j + CM_W * CM_H * k; }

static bool same_tables(const CmTables &a, const CmTables &b)
{
    bool same = a.cap_pool == b.cap_pool && a.n_valid == b.n_valid;
    for (int k = 0; k < 3; ++k) same = same && a.cen[k] == b.cen[k];
    for (int v = 0; v < a.n_valid && same; ++v) same = a.valid[v] == b.valid[v];
    for (int w = 0; w < 2; ++w) same = same && a.top[w] == b.top[w] && a.cur[w] == b.cur[w] && a.off[w] == b.off[w] && a.cnt[w] == b.cnt[w];
    return same;
}

// ---------------------------------------------------------------- the model
struct Model {
    std::vector<int> cloud[2][CM_N];
    int cen[3] = {10, 10, 5};

    // laserMapping.cpp:1598-1778: along one row of the array every cloud moves one cube up (dir > 0) or down, the one that falls
    // off the end is cleared and comes back in at the other end
    void shift(int axis, int dir)
    {
        const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
        for (int w = 0; w < 2; ++w)
            for (int u = 0; u < DIM[a1]; ++u) for (int v = 0; v < DIM[a2]; ++v) {
                int idx[3];
                idx[a1] = u; idx[a2] = v;
                std::vector<std::vector<int>> row(DIM[axis]);
                for (int i = 0; i < DIM[axis]; ++i) { idx[axis] = i; row[i] = cloud[w][cube_at(idx[0], idx[1], idx[2])]; }
                if (dir > 0) { row.pop_back(); row.insert(row.begin(), std::vector<int>()); }
                else { row.erase(row.begin()); row.push_back(std::vector<int>()); }
                for (int i = 0; i < DIM[axis]; ++i) { idx[axis] = i; cloud[w][cube_at(idx[0], idx[1], idx[2])] = row[i]; }
            }
    }

    // :1584-1593 for translations that are no multiple of 50 m, then the shift loops: the centre cube ends up 3 cubes inside
    void recentre(const double t[3], int cc[3])
    {
        for (int k = 0; k < 3; ++k) {
            cc[k] = (int)std::floor((t[k] + 25.0) / 50.0) + cen[k];
            while (cc[k] < 3) { shift(k, +1); ++cc[k]; ++cen[k]; }
            while (cc[k] >= DIM[k] - 3) { shift(k, -1); --cc[k]; --cen[k]; }
        }
    }

    // :1783-1801: the cubes at most 2, 2, 1 away from cc, ordered by i, then j, then k
    static std::vector<int> valid(const int cc[3])
    {
        std::vector<std::tuple<int, int, int>> ijk;
        for (int c = 0; c < CM_N; ++c) {
            const int i = c % CM_W, j = c / CM_W % CM_H, k = c / (CM_W * CM_H);
            if (std::abs(i - cc[0]) <= 2 && std::abs(j - cc[1]) <= 2 && std::abs(k - cc[2]) <= 1) ijk.emplace_back(i, j, k);
        }
        std::sort(ijk.begin(), ijk.end());
        std::vector<int> out;
        for (const auto &t : ijk) out.push_back(cube_at(std::get<0>(t), std::get<1>(t), std::get<2>(t)));
        return out;
    }
};

static std::vector<int> every_second(const std::vector<int> &ids)
{
    std::vector<int> out;
    for (size_t i = 0; i < ids.size(); i += 2) out.push_back(ids[i]);
    return out;
}

// ---------------------------------------------------------------- tables + pools driven against the model
struct Rig {
    CmTables T;
    Model M;
    std::vector<int> pool[2][2];
    std::mt19937 rng;
    int next_id = 0;
    long frames = 0, refused = 0, compactions = 0, grown = 0, merges = 0, shifts = 0;

    Rig(size_t cap, unsigned seed) : rng(seed)
    {
        T.cap_pool = cap;
        for (int w = 0; w < 2; ++w) for (int b = 0; b < 2; ++b) pool[w][b].assign(cap, -1);
    }
    int pick(int n) { return (int)(rng() % (unsigned)n); }

    // every cube's range holds the model's ids; the live ranges are disjoint and lie below top <= cap_pool
    void check_state(const char *when)
    {
        CHECK(T.cen[0] == M.cen[0] && T.cen[1] == M.cen[1] && T.cen[2] == M.cen[2], "%s frame %ld: centre", when, frames);
        for (int w = 0; w < 2; ++w) {
            CHECK(T.top[w] <= T.cap_pool, "%s frame %ld type %d: top %zu above cap_pool", when, frames, w, T.top[w]);
            std::vector<char> used(T.cap_pool, 0);
            for (int c = 0; c < CM_N; ++c) {
                const std::vector<int> &want = M.cloud[w][c];
                CHECK(T.cnt[w][c] == (int)want.size(), "%s frame %ld type %d cube %d: %d points, the model has %zu", when, frames, w, c, T.cnt[w][c], want.size());
                if (want.empty()) continue;
                CHECK(T.off[w][c] >= 0 && (size_t)T.off[w][c] + want.size() <= T.top[w], "%s frame %ld type %d cube %d: range beyond top", when, frames, w, c);
                for (size_t i = 0; i < want.size(); ++i) {
                    const size_t at = (size_t)T.off[w][c] + i;
                    CHECK(!used[at], "%s frame %ld type %d cube %d: overlaps another cube", when, frames, w, c);
                    used[at] = 1;
                    CHECK(pool[w][T.cur[w]][at] == want[i], "%s frame %ld type %d cube %d point %zu: id %d, the model has %d", when, frames, w, c, i, pool[w][T.cur[w]][at], want[i]);
                }
            }
        }
    }

    // what the library's copy kernels do with a piece: the old cloud out of `from`, then the new points through the sorted order
    static void apply(const std::vector<CmPiece> &pieces, const std::vector<int> &from, const std::vector<int> &sorted, std::vector<int> &to, std::vector<char> *written)
    {
        for (const CmPiece &e : pieces)
            for (int i = 0; i < e.old_cnt + e.new_cnt; ++i) {
                const size_t dst = (size_t)e.dst + i;
                CHECK(dst < to.size(), "a piece of cube %d writes beyond its destination", e.cube);
                if (written) { CHECK(!(*written)[dst], "two pieces write the same place"); (*written)[dst] = 1; }
                to[dst] = i < e.old_cnt ? from.at((size_t)e.old_off + i) : sorted.at((size_t)e.new_first + (i - e.old_cnt));
                CHECK(to[dst] >= 0, "a piece of cube %d reads a dead point", e.cube);
            }
    }

    // one frame.  merge: the set is the cubes with new points, ascending (ll_cubemaps_merge); else prepare at t and the valid cubes
    void frame(const double t[3], bool merge)
    {
        ++frames;
        if (!merge) {
            int cc[3], mc[3];
            const CmTables before = T;
            cm_follow(T, t);
            cm_centre(T, t, cc);                                     // after the shifts: the centre cube in the new indices
            M.recentre(t, mc);
            if (!(before.off[0] == T.off[0] && before.cnt[0] == T.cnt[0])) ++shifts;
            CHECK(cc[0] == mc[0] && cc[1] == mc[1] && cc[2] == mc[2], "frame %ld: centre cube", frames);
            for (int k = 0; k < 3; ++k) CHECK(cc[k] >= 3 && cc[k] < DIM[k] - 3, "frame %ld: the centre cube is not 3 cubes inside", frames);
            const std::vector<int> want = Model::valid(mc);
            CHECK(want.size() == 75 && want == std::vector<int>(T.valid, T.valid + T.n_valid), "frame %ld: valid list", frames);
            check_state("after the shifts of");
        }
        // new points in "stack order": into set cubes, other cubes of the array, or outside the array (key CM_N: sorted last, not counted)
        std::vector<std::pair<int, int>> stack[2];                   // (cube key, id)
        std::vector<int> sorted[2], addcnt[2];
        for (int w = 0; w < 2; ++w) {
            const int n = pick(4) == 0 ? 0 : pick(48);
            for (int i = 0; i < n; ++i) {
                const int kind = pick(20);
                int key;
                if (kind < 12 && T.n_valid > 0) key = T.valid[pick(T.n_valid)];
                else if (kind < 15) key = pick(CM_N);
                else if (kind < 18) { const int far[4] = {2428, 2422, 2488, 77}; key = far[pick(4)]; }      // a few cubes that keep growing
                else key = CM_N;
                if (merge && key == CM_N && pick(2)) key = pick(CM_N);
                stack[w].emplace_back(key, next_id++);
            }
            std::stable_sort(stack[w].begin(), stack[w].end(), [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first < b.first; });
            addcnt[w].assign(CM_N + 1, 0);
            for (const auto &p : stack[w]) { sorted[w].push_back(p.second); if (p.first < CM_N) ++addcnt[w][p.first]; }
        }
        // plan -> filter input -> "filter"
        CmPlan plan[2];
        std::vector<int> seg_count[2], out[2], sets[2];
        std::vector<char> member[2];
        std::vector<std::vector<int>> fresh[2];                      // per cube of the array: its new ids in stack order
        for (int w = 0; w < 2; ++w) {
            fresh[w].assign(CM_N, std::vector<int>());
            for (const auto &p : stack[w]) if (p.first < CM_N) fresh[w][p.first].push_back(p.second);
            std::vector<int> &set = sets[w];
            set.assign(T.valid, T.valid + T.n_valid);
            if (merge) { set.clear(); for (int c = 0; c < CM_N; ++c) if (addcnt[w][c] > 0) set.push_back(c); }
            const CmPlan &P = plan[w] = cm_plan(T, w, set.data(), (int)set.size(), addcnt[w].data());
            CHECK(P.seg_off.size() == set.size() + 1 && P.seg_off[0] == 0 && P.goff.size() == CM_N + 1, "frame %ld: plan shape", frames);
            for (int c = 0, g = 0; c < CM_N; g += addcnt[w][c++]) CHECK(P.goff[c] == g, "frame %ld: goff of cube %d", frames, c);
            std::vector<int> grown;
            member[w].assign(CM_N, 0);
            for (const int c : set) member[w][c] = 1;
            for (int c = 0; c < CM_N; ++c) if (!member[w][c] && !fresh[w][c].empty()) grown.push_back(c);
            CHECK(P.grown == grown, "frame %ld: the cubes outside the set that received points", frames);
            std::vector<int> in((size_t)P.seg_off.back(), -1);
            std::vector<char> written(in.size(), 0);
            apply(P.pieces, pool[w][T.cur[w]], sorted[w], in, &written);
            int longest = 0;
            for (size_t s = 0; s < set.size(); ++s) {
                std::vector<int> want = M.cloud[w][set[s]];
                want.insert(want.end(), fresh[w][set[s]].begin(), fresh[w][set[s]].end());
                CHECK(P.seg_off[s + 1] - P.seg_off[s] == (int)want.size(), "frame %ld type %d: segment %zu length", frames, w, s);
                CHECK(std::equal(want.begin(), want.end(), in.begin() + P.seg_off[s]), "frame %ld type %d: segment %zu is not the cube's cloud then its new points", frames, w, s);
                const std::vector<int> kept = every_second(want);
                longest = std::max(longest, (int)want.size());
                seg_count[w].push_back((int)kept.size());
                out[w].insert(out[w].end(), kept.begin(), kept.end());
            }
            CHECK(cm_max_segment(P.seg_off) == longest, "frame %ld: longest segment", frames);
        }
        // fit: both types before either commits; the model's own statement of the rule
        const CmTables before = T;
        size_t need[2] = {0, 0};
        bool fits = true;
        for (int w = 0; w < 2; ++w) {
            size_t want_need = out[w].size(), live = 0;
            for (int c = 0; c < CM_N; ++c) {
                if (member[w][c]) continue;
                live += M.cloud[w][c].size();
                if (!fresh[w][c].empty()) want_need += M.cloud[w][c].size() + fresh[w][c].size();
            }
            const bool want_fit = !(T.top[w] + want_need > T.cap_pool * 3 / 4 && live + want_need > T.cap_pool);
            std::string err;
            const bool fit = cm_fit(T, w, plan[w], sets[w].data(), (int)sets[w].size(), addcnt[w].data(), seg_count[w].data(), &need[w], &err);
            CHECK(fit == want_fit && need[w] == want_need, "frame %ld type %d: fit %d need %zu, the model says %d %zu", frames, w, (int)fit, need[w], (int)want_fit, want_need);
            CHECK(fit == err.empty() && (fit || err == "cube map pool exhausted (pool_points too small)"), "frame %ld: refusal text '%s'", frames, err.c_str());
            fits = fits && fit;
        }
        CHECK(same_tables(before, T), "frame %ld: planning or the fit decision changed a table", frames);
        if (!fits) { ++refused; check_state("after the refused"); return; }       // the model keeps what it had, too
        // commit
        for (int w = 0; w < 2; ++w) {
            const bool compacts = T.top[w] + need[w] > T.cap_pool * 3 / 4;
            const int cur0 = T.cur[w];
            const CmCommit K = cm_commit(T, w, plan[w], sets[w].data(), (int)sets[w].size(), addcnt[w].data(), seg_count[w].data(), need[w]);
            CHECK((T.cur[w] != cur0) == compacts && (compacts || K.moves.empty()), "frame %ld type %d: compaction moment", frames, w);
            if (compacts) {
                ++compactions;
                std::vector<int> &to = pool[w][T.cur[w]], &from = pool[w][cur0];
                to.assign(T.cap_pool, -1);
                for (const CmPiece &e : K.moves) CHECK(e.new_cnt == 0, "a compaction move carries new points");
                apply(K.moves, from, sorted[w], to, nullptr);
                from.assign(T.cap_pool, -1);                       // the pool that was current is dead
            }
            std::vector<int> &cur = pool[w][T.cur[w]];
            CHECK(K.at + out[w].size() <= T.cap_pool, "frame %ld type %d: filtered block", frames, w);
            for (size_t i = 0; i < out[w].size(); ++i) { CHECK(cur[K.at + i] < 0, "the filtered block overwrites a live point"); cur[K.at + i] = out[w][i]; }
            for (size_t g = 0; g < K.grow.size(); ++g) {
                CHECK(!member[w][K.grow[g].cube] && (g == 0 || K.grow[g - 1].cube < K.grow[g].cube), "frame %ld: grow pieces ascend outside the set", frames);
                CHECK(!merge, "a merge grows no cube outside its set");
            }
            apply(K.grow, cur, sorted[w], cur, nullptr);
            grown += (long)K.grow.size();
            for (const CmPiece &e : K.grow) for (int i = 0; i < e.old_cnt; ++i) cur[(size_t)e.old_off + i] = -1;   // the old place of a grown cloud is dead
            // the model: a set cube is its cloud + new points, filtered; any other cube that received points appends them
            for (int c = 0; c < CM_N; ++c) {
                std::vector<int> &m = M.cloud[w][c];
                if (!member[w][c] && fresh[w][c].empty()) continue;
                m.insert(m.end(), fresh[w][c].begin(), fresh[w][c].end());
                if (member[w][c]) m = every_second(m);
            }
        }
        if (merge) ++merges;
        check_state("after");
    }
};

// ---------------------------------------------------------------- direct checks
static void direct_checks()
{
    // the centre cube: truncation, then one down below -25 m -- at a multiple of 50 m below zero the reference's rule gives one less than floor
    {
        CmTables T;
        const double t[][3] = {{0.0, 24.9, 25.0}, {-24.9, -25.0, -25.1}, {-75.0, -75.1, 125.0}};
        const int want[][3] = {{10, 10, 6}, {10, 10, 4}, {8, 8, 8}};
        for (int r = 0; r < 3; ++r) {
            int cc[3];
            cm_centre(T, t[r], cc);
            for (int k = 0; k < 3; ++k) CHECK(cc[k] == want[r][k], "centre cube of %g: %d, expected %d", t[r][k], cc[k], want[r][k]);
        }
    }
    // the valid list at an interior centre: 75 cubes, i outermost, k innermost; clipped at the array's faces; none far outside
    {
        int valid[125];
        const int cc[3] = {10, 10, 5};
        CHECK(cm_valid_cubes(cc, valid) == 75, "75 valid cubes at an interior centre");
        for (int i = 8; i <= 12; ++i) for (int j = 8; j <= 12; ++j) for (int k = 4; k <= 6; ++k)
            CHECK(valid[((i - 8) * 5 + (j - 8)) * 3 + (k - 4)] == cube_at(i, j, k), "valid list order at %d %d %d", i, j, k);
        const int corner[3] = {0, 20, 10}, outside[3] = {-5, 3, 3};
        CHECK(cm_valid_cubes(corner, valid) == 3 * 3 * 2 && valid[0] == cube_at(0, 18, 9), "valid cubes at a corner of the array");
        CHECK(cm_valid_cubes(outside, valid) == 0, "no valid cube around a centre far outside");
    }
    // +1 then -1 along an axis loses exactly the layer that was pushed out: the last one; -1 then +1 the first one
    for (int axis = 0; axis < 3; ++axis)
        for (int first = +1; first >= -1; first -= 2) {
            CmTables T;
            for (int w = 0; w < 2; ++w) for (int c = 0; c < CM_N; ++c) { T.off[w][c] = 7 * c + w + 1; T.cnt[w][c] = c + 1 + 5000 * w; }
            const CmTables before = T;
            cm_shift(&T, axis, first); cm_shift(&T, axis, -first);
            for (int w = 0; w < 2; ++w) for (int c = 0; c < CM_N; ++c) {
                const int idx[3] = {c % CM_W, c / CM_W % CM_H, c / (CM_W * CM_H)};
                const bool lost = idx[axis] == (first > 0 ? DIM[axis] - 1 : 0);
                CHECK(T.off[w][c] == (lost ? 0 : before.off[w][c]) && T.cnt[w][c] == (lost ? 0 : before.cnt[w][c]), "shift %+d then back on axis %d: cube %d", first, axis, c);
            }
        }
    // a plan over an all-empty set: n_valid + 1 zero offsets, no pieces
    {
        CmTables T;
        const int cc[3] = {10, 10, 5};
        T.n_valid = cm_valid_cubes(cc, T.valid);
        const std::vector<int> addcnt(CM_N + 1, 0);
        for (int w = 0; w < 2; ++w) {
            const CmPlan P = cm_plan(T, w, T.valid, T.n_valid, addcnt.data());
            CHECK(P.seg_off == std::vector<int>((size_t)T.n_valid + 1, 0) && P.pieces.empty() && P.grown.empty() && cm_max_segment(P.seg_off) == 0, "plan over empty cubes");
        }
    }
    CHECK(cm_max_segment({0, 3, 3, 10}) == 7 && cm_max_segment({0}) == 0, "longest segment");
}

int main()
{
    direct_checks();
    // a vehicle that wanders over +-1500 m (negative coordinates, shifts on all three axes, now and then a jump) in pools of 1400 points
    long frames = 0, refused = 0, compactions = 0, grown = 0, merges = 0, shifts = 0;
    for (unsigned seed = 1; seed <= 3; ++seed) {
        Rig R(1400, seed);
        double t[3] = {0.0, 0.0, 0.0};
        for (int f = 0; f < 1200; ++f) {
            const double step[3] = {40.0, 40.0, 25.0};
            if (R.pick(10) < 3) for (int k = 0; k < 3; ++k) t[k] += step[k] * ((double)R.pick(2001) / 1000.0 - 1.0) + 0.123;
            if (R.pick(150) == 0) for (int k = 0; k < 3; ++k) t[k] = (k == 2 ? 300.0 : 1500.0) * ((double)R.pick(2001) / 1000.0 - 1.0) + 0.0123;
            R.frame(t, f > 0 && R.pick(5) == 0);
        }
        frames += R.frames; refused += R.refused; compactions += R.compactions; grown += R.grown; merges += R.merges; shifts += R.shifts;
    }
    std::printf("frames %ld refused %ld compactions %ld grown cubes %ld merges %ld frames with shifts %ld\n", frames, refused, compactions, grown, merges, shifts);
    CHECK(refused >= 20 && compactions >= 20 && grown >= 200 && merges >= 100 && shifts >= 50 && frames - refused >= 1000, "the random frames did not reach every path");
    return 0;
}
