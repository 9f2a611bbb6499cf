/* The plain C++ part of sitrack_amd/csrc/sitrk_bins.h, included alone, against restatements of what the modules did before they
 * shared it: the two radix-sort end-bit loops, the trip count of the fixed-trip search, the order key of a double and its inverse.
 * Prints one line per failed check and a last line "bins_check: N checks, F failed"; exit status 1 when F > 0.
 * Build: g++ -std=c++17 -I sitrack_amd/csrc -o bins_check tests/c/bins_check.cpp */
#include <algorithm>
#include <float.h>
#include <math.h>
#include <random>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "sitrk_bins.h"

static long nchecks = 0, nfailed = 0;

#define CHECK(cond, ...)                  \
    do {                                  \
        nchecks++;                        \
        if (!(cond)) {                    \
            nfailed++;                    \
            printf("FAILED %s: ", #cond); \
            printf(__VA_ARGS__);          \
            printf("\n");                 \
        }                                 \
    } while (0)

/* the loop of the modules that sort keys 0 .. ncells - 1 (subsample, coast, delaunay's rows) ... */
static unsigned end_bit_lt(uint64_t ncells)
{
    unsigned end_bit = 1;
    while (end_bit < 32 && ((uint64_t)1 << end_bit) < ncells) end_bit++;
    return end_bit;
}

/* ... and of those that park their invalid points at key ncells (overlap, delaunay, pairs, coarse) */
static unsigned end_bit_le(uint64_t ncells)
{
    unsigned end_bit = 1;
    while (end_bit < 32 && ((uint64_t)1 << end_bit) <= ncells) end_bit++;
    return end_bit;
}

/* the trips pairs computed for its search */
static int steps_of_pairs(int64_t nvalid)
{
    int steps = 1;
    while (((int64_t)1 << steps) <= nvalid) steps++;
    return steps;
}

static uint64_t bits_of(double v)
{
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

static void check_key_bits()
{
    std::vector<uint64_t> m = {0, 1, 2, 3, 0xffffffffull};
    for (int k : {4, 16, 22, 24, 31})
        for (int d = -1; d <= 1; d++) m.push_back(((uint64_t)1 << k) + d);
    for (uint64_t max_key : m) {
        const unsigned e = sitrk::key_bits(max_key);
        CHECK(e >= 1 && e <= 32, "max_key %llu: %u", (unsigned long long)max_key, e);
        CHECK(e == 32 || ((uint64_t)1 << e) > max_key, "max_key %llu: 2^%u does not exceed it", (unsigned long long)max_key, e);
        CHECK(e == 1 || ((uint64_t)1 << (e - 1)) <= max_key, "max_key %llu: %u is not the smallest", (unsigned long long)max_key, e);
        /* a caller with keys 0 .. ncells - 1 passes ncells - 1, one with keys 0 .. ncells passes ncells */
        CHECK(e == end_bit_lt(max_key + 1), "ncells %llu, keys below it: %u, the loop %u", (unsigned long long)max_key + 1, e, end_bit_lt(max_key + 1));
        CHECK(e == end_bit_le(max_key), "ncells %llu, keys up to it: %u, the loop %u", (unsigned long long)max_key, e, end_bit_le(max_key));
    }
}

static void check_order_key()
{
    const double v[] = {-INFINITY, -1.0, -DBL_MIN, -4.9406564584124654e-324, -0.0, 0.0, 4.9406564584124654e-324, DBL_MIN, 1.0, INFINITY};
    const int n = (int)(sizeof v / sizeof v[0]);
    CHECK(bits_of(v[3]) == 0x8000000000000001ull && bits_of(v[6]) == 1ull, "the denormals of least magnitude");
    for (int i = 0; i < n; i++)
        CHECK(bits_of(sitrk::order_value(sitrk::order_key(v[i]))) == bits_of(v[i]), "round trip of %a: %a", v[i], sitrk::order_value(sitrk::order_key(v[i])));
    /* x < y <=> key(x) < key(y), but for the one pair of doubles that differ in their bits and compare equal: the keys of -0.0 and +0.0
     * are neighbours in that order (a box of zeros still comes back as zeros, of either sign) */
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < n; j++) {
            const bool lt = v[i] < v[j], klt = sitrk::order_key(v[i]) < sitrk::order_key(v[j]);
            const bool zeros = bits_of(v[i]) == bits_of(-0.0) && bits_of(v[j]) == bits_of(0.0);
            CHECK(!lt || klt, "%a < %a but the keys are not", v[i], v[j]);
            CHECK(!klt || lt || zeros, "key(%a) < key(%a) but the values are not", v[i], v[j]);
        }
    }
    CHECK(sitrk::order_key(-0.0) + 1 == sitrk::order_key(0.0), "the keys of -0.0 and +0.0 are not neighbours");
}

/* the search of bin_start_kernel with `steps` trips, over keys given by a function of the position */
template <typename Key>
static int64_t fixed_trip_lower_bound(int64_t n, int steps, uint32_t b, Key key)
{
    int64_t lo = 0, hi = n;
    for (int it = 0; it < steps; it++) {
        if (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (key(mid) < b) lo = mid + 1; else hi = mid;
        }
    }
    return lo;
}

static void check_lower_bound_steps()
{
    std::vector<int64_t> lens = {0, 1, 2, 3};
    for (int k : {4, 16, 22, 24, 31})
        for (int d = -1; d <= 1; d++) lens.push_back(((int64_t)1 << k) + d);
    std::mt19937_64 rng(12345);
    for (int64_t n : lens) {
        const int steps = sitrk::lower_bound_steps(n);
        CHECK(steps == steps_of_pairs(n), "n %lld: %d trips, pairs took %d", (long long)n, steps, steps_of_pairs(n));
        /* random sorted keys 0 .. max of that length, given by where each run begins: first[b] is the lower bound of b by
         * construction, first[0] = 0 and first[max + 1] = n; empty runs and one long run included */
        const uint32_t max = 40;
        std::vector<int64_t> first(max + 2);
        for (auto &f : first) f = n > 0 ? (int64_t)(rng() % (uint64_t)(n + 1)) : 0;
        std::sort(first.begin(), first.end());
        first[0] = 0; first[max + 1] = n;
        first[7] = first[8] = first[9];                                     /* keys 7 and 8 do not occur */
        auto key = [&](int64_t i) { return (uint32_t)(std::upper_bound(first.begin(), first.end() - 1, i) - first.begin() - 1); };
        for (uint32_t b = 0; b <= max + 1; b++)
            CHECK(fixed_trip_lower_bound(n, steps, b, key) == first[b], "n %lld, b %u: %lld, lower bound %lld", (long long)n, b,
                  (long long)fixed_trip_lower_bound(n, steps, b, key), (long long)first[b]);
        if (n <= (1 << 16) + 1) {                                           /* the same keys as an array, against std::lower_bound */
            std::vector<uint32_t> keys((size_t)n);
            for (int64_t i = 0; i < n; i++) keys[(size_t)i] = key(i);
            CHECK(std::is_sorted(keys.begin(), keys.end()), "n %lld: the keys are not sorted", (long long)n);
            for (uint32_t b = 0; b <= max + 1; b++) {
                const int64_t want = std::lower_bound(keys.begin(), keys.end(), b) - keys.begin();
                const int64_t got = fixed_trip_lower_bound(n, steps, b, [&](int64_t i) { return keys[(size_t)i]; });
                CHECK(got == want, "n %lld, b %u: %lld, std::lower_bound %lld", (long long)n, b, (long long)got, (long long)want);
            }
        }
        /* the count is not generous: the keys 0 1 1 1 ... halve the range down to position 1, and one trip fewer does not get there */
        auto step_up = [](int64_t i) { return i >= 1 ? 1u : 0u; };
        if (n > 0) {
            CHECK(fixed_trip_lower_bound(n, steps, 1, step_up) == 1, "n %lld: %d trips do not find position 1", (long long)n, steps);
            CHECK(fixed_trip_lower_bound(n, steps - 1, 1, step_up) != 1, "n %lld: %d trips would do", (long long)n, steps - 1);
        }
    }
}

int main()
{
    check_key_bits();
    check_order_key();
    check_lower_bound_steps();
    printf("bins_check: %ld checks, %ld failed\n", nchecks, nfailed);
    return nfailed ? 1 : 0;
}
