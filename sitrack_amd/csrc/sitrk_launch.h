// sitrk_launch.h -- the shapes of the library's capped launches, computed on the host.  Plain C++, nothing of HIP: a host program
// can include it alone (tests/c/launch_shape_check.cpp prints what it derives, for the tests that choose their sizes by it).
#pragma once
#include <stdint.h>

namespace sitrk {

inline unsigned nblk(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// the launch of a kernel whose lanes step a grid at a time: at most max_blocks workgroups (at least one) and the trips that cover n
struct Strided {
    unsigned blocks;
    int trips;
    Strided(int64_t n, int threads, unsigned max_blocks)
    {
        blocks = nblk(n, threads) < max_blocks ? nblk(n, threads) : max_blocks;
        if (blocks < 1) blocks = 1;
        trips = (int)((n + (int64_t)blocks * threads - 1) / ((int64_t)blocks * threads));
    }
};

// the launch of a kernel whose waves each take a span of pixels of their own: `trips` pieces of 64 pixels that follow each other,
// at least min_trips, and so many that at most span_waves waves cover npix
struct WaveSpans {
    int trips;
    unsigned blocks;
    WaveSpans(int64_t npix, int threads, int64_t span_waves, int min_trips)
    {
        const int64_t pieces = (npix + 63) / 64;
        const int64_t want = (pieces + span_waves - 1) / span_waves;
        trips = (int)(want > min_trips ? want : min_trips);
        blocks = (unsigned)(((pieces + trips - 1) / trips + threads / 64 - 1) / (threads / 64));
    }
};

}  // namespace sitrk
