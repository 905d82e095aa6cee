// The tile / segment vocabulary of the tiled kernels (csrc/ll_tiles.h) on the host alone: LLTiler's numbering against the prefix
// sums of ceil(cnt / per), and ll_tile_find against a linear scan for EVERY tile of crafted segment tables -- counts drawn from
// {1, per - 1, per, per + 1, 2 per, 5 per + 3}, tables of 1, 2, 3 (every combination) and 300 segments, per = 256 and 1024.
// Built with -fsanitize=address,undefined by tests/test_tiles_host.py; exit status 0 = everything held.
#include "ll_tiles.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond, ...)                                                                     \
    do {                                                                                     \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } \
    } while (0)

struct Seg { int cnt; unsigned tile0; };

static long long n_tables = 0, n_tiles = 0;

// the segment of tile t by definition: the one with tile0 <= t < tile0 + ceil(cnt / per); -1: none or more than one
static int linear_find(const std::vector<Seg> &segs, const std::vector<unsigned long long> &ntile, unsigned t)
{
    int found = -1;
    for (size_t s = 0; s < segs.size(); ++s)
        if (segs[s].tile0 <= t && (unsigned long long)t < segs[s].tile0 + ntile[s]) { if (found >= 0) return -1; found = (int)s; }
    return found;
}

static void check_table(int per, const std::vector<int> &counts)
{
    LLTiler T{per};
    CHECK(T.next == 0 && T.fits(), "a new tiler has handed out %llu tiles", T.next);
    std::vector<Seg> segs;
    std::vector<unsigned long long> ntile;
    unsigned long long sum = 0;
    for (const int cnt : counts) {
        const unsigned tile0 = T.take(cnt);
        const unsigned long long need = ((unsigned long long)cnt + (unsigned long long)per - 1) / (unsigned long long)per;
        CHECK(tile0 == sum, "per %d, segment %zu of %d points: tile0 %u, the segments before it hold %llu tiles", per, segs.size(), cnt, tile0, sum);
        sum += need;
        CHECK(T.next == sum, "per %d, after %zu segments: next %llu, the prefix sum is %llu", per, segs.size() + 1, T.next, sum);
        segs.push_back({cnt, tile0});
        ntile.push_back(need);
    }
    CHECK(T.fits(), "per %d: %llu tiles do not fit", per, T.next);
    const int nseg = (int)segs.size();
    std::vector<char> first_seen(nseg, 0), last_seen(nseg, 0);
    for (unsigned long long t = 0; t < T.next; ++t) {
        const int want = linear_find(segs, ntile, (unsigned)t), got = ll_tile_find(segs.data(), nseg, (unsigned)t);
        CHECK(want >= 0, "per %d, %d segments: tile %llu belongs to no segment or to two", per, nseg, t);
        CHECK(got == want, "per %d, %d segments: tile %llu is in segment %d, ll_tile_find says %d", per, nseg, t, want, got);
        if (t == segs[got].tile0) first_seen[got] = 1;
        if (t == segs[got].tile0 + ntile[got] - 1) last_seen[got] = 1;
        if (nseg == 1) CHECK(got == 0, "one segment: tile %llu gives %d", t, got);
        ++n_tiles;
    }
    for (int s = 0; s < nseg; ++s) CHECK(first_seen[s] && last_seen[s], "per %d: the first or the last tile of segment %d was not among the tiles", per, s);
    ++n_tables;
}

int main()
{
    for (const int per : {256, 1024}) {
        const int pick[6] = {1, per - 1, per, per + 1, 2 * per, 5 * per + 3};
        for (int a = 0; a < 6; ++a) {
            check_table(per, {pick[a]});
            for (int b = 0; b < 6; ++b) {
                check_table(per, {pick[a], pick[b]});
                for (int c = 0; c < 6; ++c) check_table(per, {pick[a], pick[b], pick[c]});
            }
        }
        // about 300 segments: the six counts in turn (every one is there), then in an order of their own
        std::vector<int> turn, mixed;
        unsigned x = 12345u + (unsigned)per;
        for (int s = 0; s < 300; ++s) {
            turn.push_back(pick[s % 6]);
            x = x * 1664525u + 1013904223u;
            mixed.push_back(pick[(x >> 16) % 6]);
        }
        check_table(per, turn);
        check_table(per, mixed);
        mixed.push_back(1);                                       // 301: an odd table size, a one-tile segment last
        check_table(per, mixed);
        // one segment: every t gives 0, also a t beyond its tiles (the search has nothing else to return)
        const Seg one = {5 * per + 3, 0};
        for (unsigned t = 0; t < 64; ++t) CHECK(ll_tile_find(&one, 1, t) == 0, "one segment: tile %u does not give 0", t);
        CHECK(ll_tile_find(&one, 1, 0x7fffffffu) == 0, "one segment: the last tile a launch can have does not give 0");
    }
    // fits(): the last grid size a launch takes and the first it does not, reached by setting next
    LLTiler T{1024};
    T.next = 0x7fffffffull;
    CHECK(T.fits(), "0x7fffffff tiles must fit");
    T.next = 0x80000000ull;
    CHECK(!T.fits(), "0x80000000 tiles must not fit");
    T.next = 0x7ffffffeull;
    CHECK(T.take(1024) == 0x7ffffffeu && T.next == 0x7fffffffull && T.fits(), "the last tile that fits");
    CHECK(T.take(1) == 0x7fffffffu && !T.fits(), "one tile more does not fit");
    std::printf("tables %lld tiles %lld\n", n_tables, n_tiles);
    return 0;
}
