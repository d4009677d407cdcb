// sim3_atan2_check.cpp -- the largest difference between orbx_sim3_atan2 (csrc/orbx_sim3.h) and the C library's atan2 over a
// dense sweep of (|v|, q0) = (sin a, cos a), a in [0, pi]: the arguments ComputeSim3 hands it.  Stand-alone, no GPU:
//   g++ -std=c++17 -O2 -ffp-contract=off -I include tools/sim3_atan2_check.cpp -o sim3_atan2_check && ./sim3_atan2_check [points]
// Prints the largest absolute difference, where it occurs, and the same in units of the last place of the libm value.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_sim3.h"

int main(int argc, char **argv) {
    const long n = argc > 1 ? atol(argv[1]) : 20000000L;
    double worst = 0.0, worst_a = 0.0, worst_ulp = 0.0;
    for (long i = 0; i <= n; ++i) {
        const double a = M_PI * (double)i / (double)n;
        const double y = std::fabs(std::sin(a)), x = std::cos(a);
        const double want = std::atan2(y, x), got = orbx_sim3_atan2_pos(y, x);
        const double d = std::fabs(got - want);
        if (d > worst) { worst = d; worst_a = a; }
        const double ulp = want > 0 ? std::nextafter(want, 4.0) - want : 0x1p-1074;
        if (d / ulp > worst_ulp) worst_ulp = d / ulp;
    }
    // the axes and the corners of the unit square, exactly
    const double ax[][2] = {{0.0, 1.0}, {0.0, -1.0}, {1.0, 0.0}, {0.0, 0.0}, {1.0, 1.0}, {1.0, -1.0}};
    for (const auto &p : ax) {
        const double d = std::fabs(orbx_sim3_atan2_pos(p[0], p[1]) - std::atan2(p[0], p[1]));
        if (d > worst) { worst = d; worst_a = std::atan2(p[0], p[1]); }
    }
    printf("points %ld  largest |orbx_sim3_atan2 - atan2| = %.3e (= 2^%.2f) at angle %.17g  largest in ulp of the libm value = %.2f\n", n + 1, worst,
           worst > 0 ? std::log2(worst) : -INFINITY, worst_a, worst_ulp);
    return 0;
}
