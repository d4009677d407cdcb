// tests/compat_pose/check.cpp -- syntax check of compat/Optimizer_pose.inl (tests/test_compat_pose.py compiles it with
// -fsyntax-only).  The shared stand-in headers (tests/compat_stubs, tests/compat_runtime) declare no Optimizer, no
// MapPoint::mGlobalMutex and no Frame::SetPose, so this file declares the few members the body touches itself, as the
// reference's include/Frame.h, include/MapPoint.h and include/Optimizer.h declare them, over the cv stand-in of
// tests/compat_runtime and the real compat/ORBextractor.h.
#include <mutex>
#include <stdexcept>
#include <vector>
#include <opencv2/core/core.hpp>
#include "ORBextractor.h"
#include "orbx.h"
namespace ORB_SLAM2 {
class MapPoint {
public:
    cv::Mat GetWorldPos();
    static std::mutex mGlobalMutex;
};
class Frame {
public:
    void SetPose(cv::Mat Tcw);
    ORBextractor *mpORBextractorLeft;
    float fx, fy, cx, cy, mbf;
    int N;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    cv::Mat mTcw;
    std::vector<float> mvInvLevelSigma2;
};
class Optimizer {
public:
    int static PoseOptimization(Frame *pFrame);
};
#include "Optimizer_pose.inl"
}  // namespace ORB_SLAM2
