// The mapping vote's threshold constants (light-loam_amd/csrc/ll_exact_math.h) against the host libm, over ranges of non-negative
// float bit patterns.  Built by tests/test_map_vote_cases.py with g++ -ffp-contract=off.
#include <math.h>
#include <stdint.h>

#include "ll_exact_math.h"

extern "C" {

/* (double)expf(-g2 / (1 * 1)) < 0.95  ==  ll_map_vote_incompatible(g2)  for the patterns first, first + stride, ... <= +inf; returns the mismatches */
long long mv_check_vote(unsigned long long first, unsigned long long stride)
{
    long long bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (long long u = (long long)first; u <= 0x7f800000LL; u += (long long)stride) {
        const float g2 = ll_u2f((uint32_t)u);
        const float resolution = 1;
        const float score = expf(-g2 / (resolution * resolution));
        const bool ref = score < 0.95;                       /* float against a double literal, as laserMapping.cpp:937 */
        if (ref != ll_map_vote_incompatible(g2)) bad++;
    }
    return bad;
}

/* ll_map_vote_incompatible_gap(g) == ll_map_vote_incompatible(RN(g * g)) */
long long mv_check_vote_gap(unsigned long long first, unsigned long long stride)
{
    long long bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (long long u = (long long)first; u <= 0x7f800000LL; u += (long long)stride) {
        const float g = ll_u2f((uint32_t)u);
        volatile float g2 = g * g;
        if (ll_map_vote_incompatible(g2) != ll_map_vote_incompatible_gap(g)) bad++;
    }
    return bad;
}

/* the smallest non-negative pattern at which each predicate's libm statement turns true (what the constants must equal) */
unsigned mv_first_incompatible_gap2(void)
{
    uint32_t lo = 0, hi = 0x7f800000u;                       /* monotone (mv_check_vote shows it): bisection */
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const float score = expf(-ll_u2f(mid));
        if (score < 0.95) hi = mid; else lo = mid + 1;
    }
    return lo;
}

}  // extern "C"
