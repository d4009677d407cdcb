// plan_split.cpp -- orbx_split_batch (csrc/orbx_internal.h), the sub-batch offsets of the sub-batch pipeline and of the
// FAST-first plan of run_chunk: every batch size, sub-batch count and head mode.  Host only; built with
// -fsanitize=address,undefined by tests/test_plan_split.py.
#include <cstdio>
#include "../orb_slam2_detailed_comments_amd/csrc/orbx_internal.h"

int main() {
    long fails = 0, cases = 0;
    for (int B = 8; B <= 1100; ++B)
        for (int S = 1; S <= 8; ++S)
            for (int head = 0; head < 2; ++head) {
                int off[ORBX_PIPE_MAX + 1];
                const int n = orbx_split_batch(B, S, head != 0, off);
                bool ok = n >= 1 && n <= S && off[0] == 0 && off[n] == B;       // from 0 to B
                for (int k = 0; ok && k < n; ++k) {
                    ok = off[k + 1] > off[k]                                     // strictly increasing
                         && (k + 1 == n || off[k + 1] % 8 == 0)                  // a multiple of 8, except the last
                         && off[k + 1] - off[k] >= 8;                            // no sub-batch under 8 frames
                }
                ++cases;
                if (!ok && ++fails <= 20) printf("FAIL B=%d S=%d head=%d n=%d\n", B, S, head, n);
            }
    printf("%ld cases, %ld failures\n", cases, fails);
    return fails != 0;
}
