/* What the library's host code derives for its capped launches (sitrack_amd/csrc/sitrk_launch.h), printed for the tests that
 * choose their raster sizes by it.  The arguments are any number of groups
 *     s N THREADS MAX_BLOCKS               -> Strided:   "blocks trips"
 *     w NPIX THREADS SPAN_WAVES MIN_TRIPS  -> WaveSpans: "blocks trips"
 * one line of output per group; exit status 2 on a malformed argument list.
 * Build: g++ -std=c++17 -I sitrack_amd/csrc -o launch_shape_check tests/c/launch_shape_check.cpp */
#include <stdio.h>
#include <stdlib.h>

#include "sitrk_launch.h"

int main(int argc, char **argv)
{
    int k = 1;
    while (k < argc) {
        const char kind = argv[k][0];
        const int need = kind == 's' ? 3 : kind == 'w' ? 4 : -1;
        if (need < 0 || argv[k][1] != 0 || k + need >= argc) return 2;
        long long a[4] = {0, 0, 0, 0};
        for (int q = 0; q < need; q++) a[q] = atoll(argv[k + 1 + q]);
        if (kind == 's') {
            const sitrk::Strided s(a[0], (int)a[1], (unsigned)a[2]);
            printf("%u %d\n", s.blocks, s.trips);
        } else {
            const sitrk::WaveSpans w(a[0], (int)a[1], a[2], (int)a[3]);
            printf("%u %d\n", w.blocks, w.trips);
        }
        k += 1 + need;
    }
    return 0;
}
