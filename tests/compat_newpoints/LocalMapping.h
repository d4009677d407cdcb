// tests/compat_newpoints: a LocalMapping with the members compat/LocalMapping_newpoints.inl touches -- mpCurrentKeyFrame, mpMap,
// mlpRecentAddedMapPoints -- and a member function that holds, for ONE neighbour, what LocalMapping::CreateNewMapPoints holds
// where its per-match loop starts (the pose copies of both keyframes, vMatchedIndices, nnew), with the fragment in the loop's place.
// KeyFrame, MapPoint and Map are recorders with the members the fragment uses: a MapPoint keeps its position, its observations
// and the calls made on it, a keyframe its slots.  cv::Mat and cv::KeyPoint come from tests/compat_runtime.
#pragma once
#include <cstdint>
#include <list>
#include <stdexcept>
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
#include "orbx.h"
namespace ORB_SLAM2 {
using namespace std;
class KeyFrame;
class Map;
class MapPoint {
public:
    MapPoint(const cv::Mat &Pos, KeyFrame *pRefKF, Map *pMap) : mWorldPos(Pos.clone()), mpRefKF(pRefKF), mpMap(pMap) {}
    void AddObservation(KeyFrame *pKF, size_t idx) { mObservations.push_back(make_pair(pKF, idx)); }
    void ComputeDistinctiveDescriptors() { mnDistinctive++; }
    void UpdateNormalAndDepth() { mnNormal++; }
    cv::Mat mWorldPos;
    KeyFrame *mpRefKF;
    Map *mpMap;
    vector<pair<KeyFrame *, size_t> > mObservations;
    int mnDistinctive = 0, mnNormal = 0;
};
class Map {
public:
    void AddMapPoint(MapPoint *pMP) { mvpMapPoints.push_back(pMP); }
    vector<MapPoint *> mvpMapPoints;
};
class KeyFrame {
public:
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints.at(idx) = pMP; }
    float fx, fy, cx, cy, invfx, invfy, mbf, mb;
    vector<cv::KeyPoint> mvKeys, mvKeysUn;
    vector<float> mvuRight, mvDepth;
    float mfScaleFactor;
    vector<float> mvScaleFactors, mvLevelSigma2;
    vector<MapPoint *> mvpMapPoints;
    cv::Mat Rcw, tcw, Ow;
};
class LocalMapping {
public:
    LocalMapping(Map *pMap, KeyFrame *pKF) : mpMap(pMap), mpCurrentKeyFrame(pKF) {}
    // one pass of the neighbour loop from where SearchForTriangulation has returned; returns nnew
    int CreateNewMapPointsFor(KeyFrame *pKF2, const vector<pair<size_t, size_t> > &vMatchedIndices)
    {
        cv::Mat Rcw1 = mpCurrentKeyFrame->GetRotation();
        cv::Mat tcw1 = mpCurrentKeyFrame->GetTranslation();
        cv::Mat Ow1 = mpCurrentKeyFrame->GetCameraCenter();
        cv::Mat Ow2 = pKF2->GetCameraCenter();
        cv::Mat Rcw2 = pKF2->GetRotation();
        cv::Mat tcw2 = pKF2->GetTranslation();
        int nnew = 0;
#include "LocalMapping_newpoints.inl"
        return nnew;
    }
    Map *mpMap;
    KeyFrame *mpCurrentKeyFrame;
    list<MapPoint *> mlpRecentAddedMapPoints;
};
}  // namespace ORB_SLAM2
