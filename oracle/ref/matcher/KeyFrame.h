// oracle/ref/matcher: stand-in for the reference's include/KeyFrame.h, for compiling src/ORBmatcher.cc and src/MapPoint.cc
// unmodified (forced in with -include; the guard makes the reference's own KeyFrame.h expand to nothing).  Members and rules:
// those of tests/compat_runtime/KeyFrame.h (each with the lines of src/KeyFrame.cc it restates), plus mnFrameId and
// GetFeaturesInArea(x, y, r), which is the restated grid (grid.h) without a level filter.  A keyframe is never bad here.
#ifndef KEYFRAME_H
#define KEYFRAME_H
#include <cmath>
#include <set>
#include <vector>
#include <opencv2/core/core.hpp>
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"
#include "grid.h"
namespace ORB_SLAM2 {
class MapPoint;
class KeyFrame {
public:
    KeyFrame(long unsigned int id, int n, int levels, float scaleFactor)
        : mnId(id), mnFrameId(id), N(n), mvpMapPoints((size_t)n, static_cast<MapPoint *>(NULL)), mnScaleLevels(levels),
          mfScaleFactor(scaleFactor), mfLogScaleFactor(std::log(scaleFactor)) {
        ScaleTables(levels, scaleFactor, mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2);
    }
    static void ScaleTables(int levels, float f, std::vector<float> &sf, std::vector<float> &s2, std::vector<float> &is2) {
        sf.assign((size_t)levels, 1.f); s2.assign((size_t)levels, 1.f); is2.assign((size_t)levels, 1.f);
        for (int l = 1; l < levels; ++l) { sf[l] = sf[l - 1] * f; s2[l] = sf[l] * sf[l]; }
        for (int l = 0; l < levels; ++l) is2[l] = 1.0f / s2[l];
    }

    void SetPose(const cv::Mat &Tcw_) {
        Tcw = Tcw_.clone();
        const cv::Mat Rcw = Tcw.rowRange(0, 3).colRange(0, 3), tcw = Tcw.rowRange(0, 3).col(3);
        Ow = -Rcw.t() * tcw;
    }
    cv::Mat GetPose() { return Tcw.clone(); }
    cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    bool isBad() { return false; }

    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::set<MapPoint *> GetMapPoints();                              // needs MapPoint::isBad: body in harness.cpp
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints.at(idx); }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints.at(idx) = pMP; }
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { mvpMapPoints.at(idx) = pMP; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints.at(idx) = static_cast<MapPoint *>(NULL); }
    bool IsInImage(const float &x, const float &y) const { return x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY; }
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r) const {
        return grid.Query(mvKeysUn, (float)mnMinX, (float)mnMaxX, (float)mnMinY, (float)mnMaxY, x, y, r, -1, -1);
    }

    long unsigned int mnId, mnFrameId;
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f, invfx = 0.f, invfy = 0.f, mbf = 0.f, mb = 0.f;
    int N;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;
    std::vector<MapPoint *> mvpMapPoints;
    int mnScaleLevels;
    float mfScaleFactor, mfLogScaleFactor;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    RefGrid grid;

private:
    cv::Mat Tcw, Ow;
};
}  // namespace ORB_SLAM2
#endif
