// tests/compat_runtime: a working Frame with the members compat/ORBmatcher.h and compat/Frame_stereo.inl touch (the member list
// of tests/compat_stubs/Frame.h).  The two member functions get their bodies from compat/Frame_stereo.inl (harness.cpp includes
// it); the image bounds are static, as in ORB-SLAM2's Frame (defined in map_model.cpp).
#pragma once
#include <map>
#include <vector>
#include <opencv2/core/core.hpp>
#include "ORBextractor.h"
#include "MapPoint.h"
namespace DBoW2 { class FeatureVector : public std::map<unsigned int, std::vector<unsigned int> > {}; }
namespace ORB_SLAM2 {
class Frame {
public:
    void ComputeStereoMatches();
    void UndistortKeyPoints();
    ORBextractor *mpORBextractorLeft = NULL, *mpORBextractorRight = NULL;
    cv::Mat mK, mDistCoef;
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f, invfx = 0.f, invfy = 0.f, mbf = 0.f, mb = 0.f;
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    DBoW2::FeatureVector mFeatVec;
    cv::Mat mDescriptors, mDescriptorsRight;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    cv::Mat mTcw;
    int mnScaleLevels = 8;
    float mfScaleFactor = 1.2f, mfLogScaleFactor = 0.f;
    std::vector<float> mvScaleFactors, mvInvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    static float mnMinX, mnMaxX, mnMinY, mnMaxY;
};
}  // namespace ORB_SLAM2
