// oracle/ref: stand-in for the reference's include/KeyFrame.h, for compiling its src/KeyFrameDatabase.cc unmodified.
// KeyFrameDatabase.h includes "KeyFrame.h" with quotes, which finds its own sibling first; this file is therefore forced in
// ahead of it (-include) and defines the sibling's include guard, so that the sibling expands to nothing.
// Members: exactly what KeyFrameDatabase.cc touches.  As in src/KeyFrame.cc:53-56 the marks and word counts start at 0.
// mLoopScore and mRelocScore, which the reference leaves uninitialised and may read before any query wrote them
// (rule F8), START AT 0.0f HERE: that makes such a read deterministic, with the value the model
// (tests/kfdb_model.py) and the library define for it.
#ifndef KEYFRAME_H
#define KEYFRAME_H
#include <set>
#include <vector>
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
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
    float mLoopScore = 0.0f;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0.0f;
    std::set<KeyFrame *> connected;      // filled by the harness
    std::vector<KeyFrame *> ordered;     // covisible keyframes, best first
};
}  // namespace ORB_SLAM2
#endif
