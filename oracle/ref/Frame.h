// oracle/ref: stand-in for the reference's include/Frame.h (see KeyFrame.h beside it for how it gets in): the two members
// KeyFrameDatabase::DetectRelocalizationCandidates reads.
#ifndef FRAME_H
#define FRAME_H
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
namespace ORB_SLAM2 {
class Frame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};
}  // namespace ORB_SLAM2
#endif
