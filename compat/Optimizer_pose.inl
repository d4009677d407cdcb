// compat/Optimizer_pose.inl -- replacement BODY for Optimizer::PoseOptimization(Frame *pFrame) (reference
// src/Optimizer.cc:363-607), the motion-only optimisation Tracking runs after every matcher call (TrackReferenceKeyFrame,
// TrackWithMotionModel, TrackLocalMap, Relocalization).
//
// How to apply (maintainer, inside the ORB-SLAM2 tree; needs OpenCV): in src/Optimizer.cc, delete the body of
// Optimizer::PoseOptimization and put   #include "Optimizer_pose.inl"   in its place, inside namespace ORB_SLAM2, with <vector>,
// <mutex>, <stdexcept> and "orbx.h" included above it.  The g2o includes of that function are no longer needed by it.  This
// repository has no stand-in for Optimizer, MapPoint::mGlobalMutex or Frame::SetPose in its shared stand-in headers; the body is
// syntax-checked against the small stand-ins of tests/compat_pose/ and the maintainer's build remains the final check.
//
// The body marshals the Frame exactly as the reference reads it: under MapPoint::mGlobalMutex it snapshots GetWorldPos() of
// every feature's MapPoint (feature order, which is the reference's edge order), passes mvKeysUn, mvuRight (< 0: a monocular
// edge), mvInvLevelSigma2, fx, fy, cx, cy, mbf and mTcw, and writes mvbOutlier for the features that have a MapPoint.  With fewer
// than 3 correspondences it returns 0 and leaves the pose alone, as the reference does; otherwise it calls SetPose with the
// optimised pose and returns the number of inliers.  One frame is one call on the library's host path (measured: one problem per
// call takes 0.24-3.3 ms on the device against 53-586 us on the host, profiles/pose_batch.md).  A tracker that holds a device batch of frames calls
// orbx_pose_optimization_batch_device on the matchers' rows instead.
// Parity: the result equals tests/pose_model.py bit for bit; parity with the g2o + Eigen body is not pinned (DESIGN.md section 2,
// F11).
int Optimizer::PoseOptimization(Frame *pFrame)
{
    const int N = pFrame->N;
    if (N <= 0) return 0;
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint must be the 28-byte POD");
    std::vector<int32_t> point((size_t)N, -1);
    std::vector<float> world;
    world.reserve((size_t)N * 3);
    {
        std::unique_lock<std::mutex> lock(MapPoint::mGlobalMutex);
        for (int i = 0; i < N; i++) {
            MapPoint *pMP = pFrame->mvpMapPoints[i];
            if (!pMP) continue;
            const cv::Mat Xw = pMP->GetWorldPos();
            point[i] = (int32_t)(world.size() / 3);
            world.push_back(Xw.at<float>(0)); world.push_back(Xw.at<float>(1)); world.push_back(Xw.at<float>(2));
        }
    }
    const int npool = (int)(world.size() / 3);
    if (npool == 0) return 0;                             // nInitialCorrespondences == 0
    float Tcw[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) Tcw[4 * r + c] = pFrame->mTcw.at<float>(r, c);
    const float camera4[4] = {pFrame->fx, pFrame->fy, pFrame->cx, pFrame->cy};
    std::vector<uint8_t> outlier((size_t)N, 0);
    int32_t ninliers = 0;
    const orbx_status st = orbx_pose_optimization(
        pFrame->mpORBextractorLeft->handle(), Tcw, N, reinterpret_cast<const orbx_keypoint *>(pFrame->mvKeysUn.data()),
        pFrame->mvuRight.data(), point.data(), npool, world.data(), camera4, pFrame->mbf, pFrame->mvInvLevelSigma2.data(),
        (int)pFrame->mvInvLevelSigma2.size(), outlier.data(), &ninliers);
    if (st != ORBX_OK) throw std::runtime_error(orbx_last_error());
    for (int i = 0; i < N; i++)
        if (point[i] >= 0) pFrame->mvbOutlier[i] = outlier[i] != 0;
    if (npool < 3) return 0;                              // the reference returns before SetPose
    cv::Mat pose(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) pose.at<float>(r, c) = Tcw[4 * r + c];
    pFrame->SetPose(pose);
    return ninliers;
}
