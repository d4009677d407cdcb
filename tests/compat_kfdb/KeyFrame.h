// tests/compat_kfdb: a KeyFrame with the members compat/KeyFrameDatabase.h touches (ORB-SLAM2 include/KeyFrame.h: mnId, mBowVec,
// the six query fields, GetConnectedKeyFrames, GetBestCovisibilityKeyFrames).  As in src/KeyFrame.cc:53-56 the marks and word
// counts start at 0; the two scores, which the reference leaves uninitialised, start as NaN so that a test sees whether the
// shim wrote them.  The covisibility graph is two plain containers the harness fills.
#pragma once
#include <cmath>
#include <set>
#include <vector>
#include "ORBVocabulary.h"
namespace ORB_SLAM2 {
class KeyFrame {
public:
    explicit KeyFrame(long unsigned int id) : mnId(id) {}
    std::set<KeyFrame *> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) {
        return (int)ordered.size() < N ? ordered : std::vector<KeyFrame *>(ordered.begin(), ordered.begin() + N);
    }
    long unsigned int mnId;
    DBoW2::BowVector mBowVec;
    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = NAN;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = NAN;
    std::set<KeyFrame *> connected;
    std::vector<KeyFrame *> ordered;
};
}  // namespace ORB_SLAM2
