// tests/compat_runtime: a working KeyFrame with the members compat/ORBmatcher.h touches (the member list of
// tests/compat_stubs/KeyFrame.h), restating ORB-SLAM2's KeyFrame where the shims depend on it:
//   SetPose                 Tcw kept; Ow = -Rcw^T tcw (src/KeyFrame.cc:113-131)
//   GetRotation / GetTranslation / GetCameraCenter / GetPose   copies of Rcw, tcw, Ow, Tcw
//   GetMapPointMatches      the slot vector, NULL and bad points included (:433-437)
//   GetMapPoints            the set of non-NULL, non-bad points of the slots (:380-397)
//   AddMapPoint / ReplaceMapPointMatch / EraseMapPointMatch   write one slot (:340-378)
//   IsInImage(x, y)         mnMinX <= x < mnMaxX and mnMinY <= y < mnMaxY (:926-929)
// The scale tables are those of ORBextractor: factor^l, its square and their inverses.  A keyframe is never bad here.
#pragma once
#include <cmath>
#include <set>
#include <vector>
#include <opencv2/core/core.hpp>
#include "MapPoint.h"
#include "Frame.h"
namespace ORB_SLAM2 {
class KeyFrame {
public:
    KeyFrame(long unsigned int id, int n, int levels, float scaleFactor)
        : mnId(id), N(n), mvpMapPoints((size_t)n, static_cast<MapPoint *>(NULL)), mnScaleLevels(levels), mfScaleFactor(scaleFactor),
          mfLogScaleFactor(std::log(scaleFactor)) {
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
    std::set<MapPoint *> GetMapPoints() {
        std::set<MapPoint *> s;
        for (size_t i = 0; i < mvpMapPoints.size(); ++i)
            if (mvpMapPoints[i] && !mvpMapPoints[i]->isBad()) s.insert(mvpMapPoints[i]);
        return s;
    }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints.at(idx); }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints.at(idx) = pMP; }
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { mvpMapPoints.at(idx) = pMP; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints.at(idx) = static_cast<MapPoint *>(NULL); }
    bool IsInImage(const float &x, const float &y) const { return x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY; }

    long unsigned int mnId;
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

private:
    cv::Mat Tcw, Ow;
};
}  // namespace ORB_SLAM2
