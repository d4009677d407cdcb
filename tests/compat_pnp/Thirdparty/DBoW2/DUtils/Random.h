// tests/compat_pnp: a stand-in for DBoW2's DUtils::Random with the one member compat/PnPsolver.h calls.  A 64-bit linear
// congruential generator (Knuth's MMIX constants) whose state the harness sets; RandomInt(min, max) = min + (state >> 33) %
// (max - min + 1) after one step.  tests/pnp_model.py (Lcg) restates it to know every draw.
#pragma once
#include <cstdint>
namespace DUtils {
class Random {
public:
    static uint64_t &State() { static uint64_t s = 1; return s; }
    static int RandomInt(int min, int max) {
        uint64_t &s = State();
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return min + (int)((s >> 33) % (uint64_t)(max - min + 1));
    }
};
}  // namespace DUtils
