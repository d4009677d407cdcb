// oracle/ref/matcher: stand-in for the reference's include/Frame.h, for compiling src/ORBmatcher.cc and src/MapPoint.cc
// unmodified (forced in with -include; the guard makes the reference's own Frame.h expand to nothing).  Members: the list of
// tests/compat_runtime/Frame.h that the two sources touch, plus mnId and GetFeaturesInArea.
// GetFeaturesInArea is NOT the reference's code (src/Frame.cc needs OpenCV's algorithms): it is the restated grid of
// oracle/orb_oracle_match.c (orc_grid_build / orc_grid_query, src/Frame.cc:633-717 with the bCheckLevels rule), built on first
// use from mvKeysUn and the static image bounds.  The order of its hits decides ties, so the grid stays a restatement.
#ifndef FRAME_H
#define FRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"
#include "grid.h"
namespace ORB_SLAM2 {
class MapPoint;
class Frame {
public:
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel = -1,
                                          const int maxLevel = -1) const {
        return grid.Query(mvKeysUn, mnMinX, mnMaxX, mnMinY, mnMaxY, x, y, r, minLevel, maxLevel);
    }
    cv::Mat GetCameraCenter() { return mOw.clone(); }                 // read by a MapPoint constructor no scene uses
    long unsigned int mnId = 0;
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f, invfx = 0.f, invfy = 0.f, mbf = 0.f, mb = 0.f;
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    DBoW2::FeatureVector mFeatVec;
    cv::Mat mDescriptors;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    cv::Mat mTcw, mOw;
    int mnScaleLevels = 8;
    float mfScaleFactor = 1.2f, mfLogScaleFactor = 0.f;
    std::vector<float> mvScaleFactors, mvInvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    static float mnMinX, mnMaxX, mnMinY, mnMaxY;
    RefGrid grid;
};
}  // namespace ORB_SLAM2
#endif
