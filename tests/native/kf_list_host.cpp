// The frame-list vocabulary of the keyframe store's consumers (csrc/ll_kf_list.h) on the host alone, at a crafted table of four
// frames with (5, 7), (0, 3), (4, 0) and (0, 0) points, offsets that leave gaps, and cap0 = 64: the pool address of all eight
// (frame, type) clouds against offsets computed by hand, the pose choice, the id refusals, the three duplicate policies, non-finite
// given and stored poses, every message against the literal string the four sites produced before they shared the check (for an
// empty side name and for "query"), first-error-wins, and the returned point total.
// Built with -fsanitize=address,undefined by tests/test_kf_list_host.py; exit status 0 = everything held.
#include "ll_kf_list.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define CHECK(cond, ...)                                                                     \
    do {                                                                                     \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } \
    } while (0)

static const long long CAP0 = 64;
static int n_checks = 0;

static std::vector<ll_keyframe_info> table()
{
    const int n[4][2] = {{5, 7}, {0, 3}, {4, 0}, {0, 0}};
    const long long off[4][2] = {{2, 1}, {9, 11}, {9, 20}, {17, 20}};      // corner: 2..6, gap, 9..12, gap; surf: 1..7, gap, 11..13, gap
    std::vector<ll_keyframe_info> tab(4);
    for (int id = 0; id < 4; ++id) {
        tab[id].lane = -1; tab[id].frame_index = id;
        for (int w = 0; w < 2; ++w) { tab[id].n[w] = n[id][w]; tab[id].offset[w] = off[id][w]; }
        for (int k = 0; k < 7; ++k) tab[id].pose_w7[k] = 100.0 * id + k;
        tab[id].pose_w7[3] = 1.0;
    }
    return tab;
}

// one check of `ids` under `dup`: the code, and msg / points as the check left them
struct Out { int rc; std::string msg; long long points; };
static Out run(const std::vector<ll_keyframe_info> &tab, int size, const std::vector<int> &ids, const double *poses, const char *side, LLKfDup dup, std::vector<int> *seen,
               int stamp, const std::string &who)
{
    Out o = {0, "untouched", -77};
    const LLKfList l = {(int)ids.size(), ids.data(), poses, side};
    o.rc = llkf_check(tab.data(), size, l, dup, seen, stamp, who, &o.msg, &o.points);
    ++n_checks;
    return o;
}

static void expect_ok(const Out &o, long long points, const char *what)
{
    CHECK(o.rc == LL_OK, "%s: refused with %d, \"%s\"", what, o.rc, o.msg.c_str());
    CHECK(o.points == points, "%s: %lld points, expected %lld", what, o.points, points);
    CHECK(o.msg == "untouched", "%s: an accepted list wrote the message \"%s\"", what, o.msg.c_str());
}

static void expect_refused(const Out &o, const std::string &text, const char *what)
{
    CHECK(o.rc == LL_ERR_ARG, "%s: code %d, expected LL_ERR_ARG", what, o.rc);
    CHECK(o.msg == text, "%s: \"%s\", expected \"%s\"", what, o.msg.c_str(), text.c_str());
    CHECK(o.points == -77, "%s: a refused list wrote the point total %lld", what, o.points);
}

int main()
{
    const std::vector<ll_keyframe_info> tab = table();
    const int size = 4;
    const LLKfDup policies[3] = {LLKF_DUP_ALLOWED, LLKF_DUP_PER_OP, LLKF_DUP_PER_CALL};
    const double nan = std::nan(""), inf = INFINITY;

    // ---- the pool address: region 1 begins at cap0
    const long long want_off[4][2] = {{2, 64 + 1}, {9, 64 + 11}, {9, 64 + 20}, {17, 64 + 20}};
    const int want_cnt[4][2] = {{5, 7}, {0, 3}, {4, 0}, {0, 0}};
    for (int id = 0; id < 4; ++id)
        for (int w = 0; w < 2; ++w) {
            const LLKfCloud c = llkf_cloud(tab.data(), CAP0, id, w);
            CHECK(c.off == want_off[id][w] && c.cnt == want_cnt[id][w], "frame %d type %d: (%lld, %d), expected (%lld, %d)", id, w, c.off, c.cnt, want_off[id][w], want_cnt[id][w]);
        }

    // ---- the pose: given row f, or the stored pose of ids[f]
    {
        const int ids[3] = {2, 0, 3};
        double given[21];
        for (int k = 0; k < 21; ++k) given[k] = -1.0 - k;
        const LLKfList with = {3, ids, given, ""}, without = {3, ids, nullptr, ""};
        for (int f = 0; f < 3; ++f) {
            CHECK(llkf_pose(tab.data(), with, f) == given + 7 * f, "given poses: entry %d is not row %d", f, f);
            CHECK(llkf_pose(tab.data(), without, f) == tab[ids[f]].pose_w7, "stored poses: entry %d is not the pose of frame %d", f, ids[f]);
        }
    }

    // ---- accepted lists and their point totals; the empty list
    for (const LLKfDup dup : policies) {
        std::vector<int> seen(size, -1);
        expect_ok(run(tab, size, {0, 1, 2, 3}, nullptr, "", dup, &seen, 0, "x: "), 5 + 7 + 3 + 4, "all four frames");
        std::fill(seen.begin(), seen.end(), -1);
        expect_ok(run(tab, size, {3}, nullptr, "", dup, &seen, 0, "x: "), 0, "the empty frame");
        expect_ok(run(tab, size, {}, nullptr, "", dup, &seen, 1, "x: "), 0, "the empty list");
        expect_ok(run(tab, size, {1, 2}, nullptr, "query", dup, &seen, 2, "x: "), 3 + 4, "two frames");
    }
    expect_ok(run(tab, size, {0, 0, 2}, nullptr, "", LLKF_DUP_ALLOWED, nullptr, 0, "x: "), 2 * 12 + 4, "a repeated frame counts twice, no scratch needed");

    // ---- ids outside the store: -1 and size, for an empty side name and for "query"; a smaller store of the same table
    for (const LLKfDup dup : policies) {
        std::vector<int> seen(size, -1);
        expect_refused(run(tab, size, {0, -1}, nullptr, "", dup, &seen, 0, "visibility: op 0: "), "visibility: op 0: frame -1 is not in the store (size 4)", "id -1");
        expect_refused(run(tab, size, {4}, nullptr, "", dup, &seen, 3, "entropy: op 3: "), "entropy: op 3: frame 4 is not in the store (size 4)", "id == size");
        expect_refused(run(tab, size, {1, 4}, nullptr, "query", dup, &seen, 1, "bev: op 1: "), "bev: op 1: query frame 4 is not in the store (size 4)", "query id == size");
        expect_refused(run(tab, size, {-1}, nullptr, "target", dup, &seen, 1, "bev: op 1: "), "bev: op 1: target frame -1 is not in the store (size 4)", "target id -1");
        expect_refused(run(tab, 3, {7}, nullptr, "query", dup, &seen, 0, "bev: op 0: "), "bev: op 0: query frame 7 is not in the store (size 3)", "query id 7 of 3");
        expect_refused(run(tab, 3, {3}, nullptr, "", dup, &seen, 0, "keyframe insert: op 0: "), "keyframe insert: op 0: frame 3 is not in the store (size 3)", "id 3 of 3");
    }

    // ---- duplicates: [0, 1, 1] in one list
    {
        std::vector<int> seen(size, -1);
        expect_ok(run(tab, size, {0, 1, 1}, nullptr, "", LLKF_DUP_ALLOWED, &seen, 0, "keyframe insert: op 0: "), 12 + 3 + 3, "[0, 1, 1], duplicates allowed");
        std::fill(seen.begin(), seen.end(), -1);
        expect_refused(run(tab, size, {0, 1, 1}, nullptr, "", LLKF_DUP_PER_OP, &seen, 0, "entropy: op 0: "), "entropy: op 0: frame 1 is listed twice in this op", "[0, 1, 1] per op");
        std::fill(seen.begin(), seen.end(), -1);
        expect_refused(run(tab, size, {0, 1, 1}, nullptr, "", LLKF_DUP_PER_CALL, &seen, 0, "visibility: op 0: "), "visibility: op 0: frame 1 is listed twice in this call", "[0, 1, 1] per call");
        std::fill(seen.begin(), seen.end(), -1);                    // the same in a later op: the stamp is the op's, not 0
        expect_refused(run(tab, size, {0, 1, 1}, nullptr, "", LLKF_DUP_PER_OP, &seen, 5, "entropy: op 5: "), "entropy: op 5: frame 1 is listed twice in this op", "[0, 1, 1] per op, op 5");
    }
    // ---- duplicates: [0, 1], [2, 0] as two ops of one call
    for (const LLKfDup dup : policies) {
        std::vector<int> seen(size, -1);
        expect_ok(run(tab, size, {0, 1}, nullptr, "", dup, &seen, 0, "x: op 0: "), 12 + 3, "[0, 1] as op 0");
        const Out second = run(tab, size, {2, 0}, nullptr, "", dup, &seen, 1, "x: op 1: ");
        if (dup == LLKF_DUP_PER_CALL) expect_refused(second, "x: op 1: frame 0 is listed twice in this call", "[2, 0] as op 1, per call");
        else expect_ok(second, 4 + 12, "[2, 0] as op 1");
    }

    // ---- non-finite poses: given and stored, NaN and Inf, component 0 and component 6
    for (const LLKfDup dup : policies)
        for (const double bad : {nan, inf, -inf})
            for (const int comp : {0, 6}) {
                std::vector<int> seen(size, -1);
                double given[14] = {0, 0, 0, 1, 1, 2, 3, 0, 0, 0, 1, 4, 5, 6};
                given[7 + comp] = bad;
                expect_refused(run(tab, size, {2, 0}, given, "", dup, &seen, 0, "entropy: op 0: "), "entropy: op 0: the pose of list entry 1 is not finite", "a given pose");
                std::fill(seen.begin(), seen.end(), -1);
                expect_refused(run(tab, size, {2, 0}, given, "query", dup, &seen, 2, "bev: op 2: "), "bev: op 2: the pose of query list entry 1 is not finite", "a given query pose");
                given[7 + comp] = 0.5;
                std::fill(seen.begin(), seen.end(), -1);
                expect_ok(run(tab, size, {2, 0}, given, "", dup, &seen, 0, "x: "), 16, "the same poses, finite");
                std::vector<ll_keyframe_info> broken = tab;
                broken[2].pose_w7[comp] = bad;
                std::fill(seen.begin(), seen.end(), -1);
                expect_refused(run(broken, size, {1, 0, 2}, nullptr, "", dup, &seen, 0, "keyframe insert: op 0: "), "keyframe insert: op 0: the pose of list entry 2 is not finite", "a stored pose");
                std::fill(seen.begin(), seen.end(), -1);
                expect_refused(run(broken, size, {2}, nullptr, "target", dup, &seen, 0, "bev: op 0: "), "bev: op 0: the pose of target list entry 0 is not finite", "a stored target pose");
                std::fill(seen.begin(), seen.end(), -1);                // a given pose stands in for the broken stored one
                expect_ok(run(broken, size, {2, 0}, given, "", dup, &seen, 0, "x: "), 16, "given poses over a broken stored pose");
            }

    // ---- the first error in list order wins; inside one entry: id, then duplicate, then pose
    {
        std::vector<ll_keyframe_info> broken = tab;
        broken[1].pose_w7[2] = nan;
        std::vector<int> seen(size, -1);
        expect_refused(run(broken, size, {0, 1, 9}, nullptr, "", LLKF_DUP_PER_CALL, &seen, 0, "v: "), "v: the pose of list entry 1 is not finite", "a bad pose before a bad id");
        std::fill(seen.begin(), seen.end(), -1);
        expect_refused(run(broken, size, {0, 9, 1}, nullptr, "", LLKF_DUP_PER_CALL, &seen, 0, "v: "), "v: frame 9 is not in the store (size 4)", "a bad id before a bad pose");
        std::fill(seen.begin(), seen.end(), -1);
        expect_refused(run(broken, size, {0, 0, 1}, nullptr, "", LLKF_DUP_PER_OP, &seen, 0, "v: "), "v: frame 0 is listed twice in this op", "a duplicate before a bad pose");
        std::fill(seen.begin(), seen.end(), -1);
        seen[1] = 0;                                                // frame 1 listed by an earlier list of the call: the duplicate comes before its pose
        expect_refused(run(broken, size, {1}, nullptr, "", LLKF_DUP_PER_CALL, &seen, 1, "v: "), "v: frame 1 is listed twice in this call", "duplicate before pose, one entry");
        expect_refused(run(broken, size, {1}, nullptr, "", LLKF_DUP_ALLOWED, nullptr, 1, "v: "), "v: the pose of list entry 0 is not finite", "no policy: the pose");
    }
    std::printf("checks %d\n", n_checks);
    return 0;
}
