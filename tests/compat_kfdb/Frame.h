// tests/compat_kfdb: the two members of ORB_SLAM2::Frame that compat/KeyFrameDatabase.h touches
#pragma once
#include "ORBVocabulary.h"
namespace ORB_SLAM2 {
class Frame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};
}  // namespace ORB_SLAM2
