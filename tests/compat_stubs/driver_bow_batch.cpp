// tests/compat_stubs: translation unit of the typo guard (g++ -fsyntax-only) for the batched SearchByBoW overloads of the
// matcher shim, written as the rewritten Relocalization / ComputeSim3 loops of INTEGRATION.md call them
#include "ORBmatcher.h"
using namespace ORB_SLAM2;
int use_bow_batch(Frame &F, KeyFrame *k1, KeyFrame *k2) {
    ORBmatcher m(0.75f, true);
    std::vector<KeyFrame *> cands(2, k2);
    std::vector<std::vector<MapPoint *> > vvpMapPointMatches;
    std::vector<int> n = m.SearchByBoWBatch(cands, F, vvpMapPointMatches);
    std::vector<std::vector<MapPoint *> > vvpMatches12;
    std::vector<int> n12 = m.SearchByBoWBatch(k1, cands, vvpMatches12);
    int total = 0;
    for (size_t i = 0; i < n.size(); ++i) total += n[i] < 15 ? 0 : (int)vvpMapPointMatches[i].size();
    for (size_t i = 0; i < n12.size(); ++i) total += n12[i] < 20 ? 0 : (int)vvpMatches12[i].size();
    return total;
}
