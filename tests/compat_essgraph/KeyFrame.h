// tests/compat_essgraph: a KeyFrame with the members compat/Optimizer_essentialgraph.inl touches (ORB-SLAM2 include/KeyFrame.h:
// mnId, isBad, GetPose, SetPose, GetParent, GetLoopEdges, GetCovisiblesByWeight, hasChild, GetWeight).  cv::Mat is the stand-in
// of tests/compat_runtime/opencv2.
#pragma once
#include <algorithm>
#include <map>
#include <set>
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame {
public:
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &T) { Tcw = T.clone(); ++nSetPose; }
    bool isBad() { return mbBad; }
    KeyFrame *GetParent() { return mpParent; }
    std::set<KeyFrame *> GetLoopEdges() { return mspLoopEdges; }
    bool hasChild(KeyFrame *pKF) { return mspChildrens.count(pKF) != 0; }
    int GetWeight(KeyFrame *pKF) { return mConnectedKeyFrameWeights.count(pKF) ? mConnectedKeyFrameWeights[pKF] : 0; }
    // mvpOrderedConnectedKeyFrames is sorted by weight, largest first; here ties keep the keyframes' order
    std::vector<KeyFrame *> GetCovisiblesByWeight(const int &w) {
        std::vector<std::pair<int, KeyFrame *> > v;
        for (std::map<KeyFrame *, int>::iterator it = mConnectedKeyFrameWeights.begin(); it != mConnectedKeyFrameWeights.end(); ++it)
            if (it->second >= w) v.push_back(std::make_pair(it->second, it->first));
        std::stable_sort(v.begin(), v.end(), [](const std::pair<int, KeyFrame *> &a, const std::pair<int, KeyFrame *> &b) { return a.first > b.first; });
        std::vector<KeyFrame *> out;
        for (size_t k = 0; k < v.size(); ++k) out.push_back(v[k].second);
        return out;
    }
    long unsigned int mnId = 0;
    cv::Mat Tcw;
    bool mbBad = false;
    KeyFrame *mpParent = NULL;
    std::set<KeyFrame *> mspLoopEdges, mspChildrens;
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    int nSetPose = 0;
};
}  // namespace ORB_SLAM2
