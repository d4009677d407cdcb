// tests/compat_sim3opt/check.cpp -- syntax check of compat/Optimizer_sim3.inl (tests/test_compat_sim3opt.py compiles it with
// -fsyntax-only).  The stand-ins of tests/compat_sim3 have no mvInvLevelSigma2 on the KeyFrame, no g2o::Sim3 and no Eigen, so
// this file declares the few members the body touches itself, as the reference's include/KeyFrame.h, include/MapPoint.h,
// include/Optimizer.h, Thirdparty/g2o/g2o/types/sim3.h and Eigen declare them, over the cv stand-in of tests/compat_runtime.
#include <stdexcept>
#include <vector>
#include <opencv2/core/core.hpp>
#include "orbx.h"
namespace Eigen {
struct Matrix3d { double operator()(int r, int c) const; };
struct Vector3d { Vector3d(double x, double y, double z); double operator[](int i) const; };
struct Quaterniond { Quaterniond(double w, double x, double y, double z); Matrix3d toRotationMatrix() const; };
}  // namespace Eigen
namespace g2o {
struct Sim3 {
    Sim3(const Eigen::Quaterniond &r, const Eigen::Vector3d &t, double s);
    const Eigen::Quaterniond &rotation() const;
    const Eigen::Vector3d &translation() const;
    const double &scale() const;
};
}  // namespace g2o
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
public:
    cv::Mat GetWorldPos();
    bool isBad();
    int GetIndexInKeyFrame(KeyFrame *pKF);
};
class KeyFrame {
public:
    cv::Mat GetRotation();
    cv::Mat GetTranslation();
    std::vector<MapPoint *> GetMapPointMatches();
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    cv::Mat mK;
};
class Optimizer {
public:
    static int OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
                            const bool bFixScale);
};
#include "Optimizer_sim3.inl"
}  // namespace ORB_SLAM2
