// oracle/ref/matcher: the feature grid behind Frame::GetFeaturesInArea and KeyFrame::GetFeaturesInArea of the stand-ins: the
// restated grid of oracle/orb_oracle_match.c, built once per view from its undistorted keypoints and image bounds.
#pragma once
#include <vector>
#include <opencv2/core/core.hpp>
extern "C" {
#include "orb_oracle.h"
}
static_assert(sizeof(orc_keypoint) == sizeof(cv::KeyPoint), "cv::KeyPoint must be the oracle's 28-byte keypoint");
namespace ORB_SLAM2 {
class RefGrid {
public:
    RefGrid() : g_(NULL) {}
    RefGrid(const RefGrid &) : g_(NULL) {}
    RefGrid &operator=(const RefGrid &) { Drop(); return *this; }
    ~RefGrid() { Drop(); }
    std::vector<size_t> Query(const std::vector<cv::KeyPoint> &keys, float minx, float maxx, float miny, float maxy, float x, float y,
                              float r, int minLevel, int maxLevel) const {
        if (!g_) g_ = orc_grid_build(reinterpret_cast<const orc_keypoint *>(keys.data()), (int)keys.size(), minx, maxx, miny, maxy);
        std::vector<int> hit(keys.size() + 1);
        const int n = orc_grid_query(g_, x, y, r, minLevel, maxLevel, hit.data(), (int)keys.size());
        return std::vector<size_t>(hit.begin(), hit.begin() + n);
    }
private:
    void Drop() { if (g_) orc_grid_free(g_); g_ = NULL; }
    mutable orc_grid *g_;
};
}  // namespace ORB_SLAM2
