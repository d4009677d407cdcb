// compat/Optimizer_sim3.inl -- replacement BODY for Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2,
// vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale) (reference
// src/Optimizer.cc:1383-1615), the optimisation LoopClosing::ComputeSim3 runs on a candidate after SearchBySim3.
//
// How to apply (maintainer, inside the ORB-SLAM2 tree; needs OpenCV, Eigen and g2o's Sim3 type): in src/Optimizer.cc, delete the
// body of Optimizer::OptimizeSim3 and put   #include "Optimizer_sim3.inl"   in its place, inside namespace ORB_SLAM2, with
// <vector>, <stdexcept> and "orbx.h" included above it.  The g2o optimizer, solver and edge includes are no longer needed by that
// function; g2o::Sim3 stays as the type of the argument.  The body is syntax-checked against the small stand-ins of
// tests/compat_sim3opt/ (the stand-ins of tests/compat_sim3 have no mvInvLevelSigma2, no g2o::Sim3 and no Eigen, so it is not
// executed there) and the maintainer's build remains the final check.
//
// The body does what the reference does around the optimisation: the pointer-chasing filters (pMP1 && pMP2, isBad,
// GetIndexInKeyFrame >= 0), the float products R1w * P3D1w + t1w as the source writes them, the call, the nulling of
// vpMatches1 (also when the call then returns 0) and the write-back of g2oS12 only when the reference assigns it.
// g2oS12 goes in as float R, t, s, which is what LoopClosing::ComputeSim3 built it from (g2o::Sim3 gScm(toMatrix3d(R),
// toVector3d(t), s)): t and s come back exactly, R goes through the quaternion and back and can differ from the solver's R in
// the last float bit.
// One candidate is one call on the library's HOST path (a host-only handle created on first use): measured on an MI355X, one
// problem per call takes 188 / 357 / 776 us on the device against 36 / 91 / 263 us on the host path for 30 / 100 / 300
// correspondences; from 16 problems per call on the device wins (14 / 26 / 57 us per problem at 16, 1.0 / 2.0 / 4.7 us at 256;
// profiles/sim3opt_batch.md).  A caller that has all candidates of a round calls orbx_optimize_sim3_batch on a device handle
// instead.
// Parity: the result equals tests/sim3opt_model.py bit for bit; parity with the g2o + Eigen body is not pinned (DESIGN.md section
// 2, F16).
int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
                            const bool bFixScale)
{
    struct HostHandle {
        orbx_handle *h = NULL;
        HostHandle() {
            orbx_params p;
            orbx_default_params(&p);
            p.device = -2;                                // host-only: the library's host path
            if (orbx_create(&p, &h) != ORBX_OK) throw std::runtime_error(orbx_last_error());
        }
        ~HostHandle() { orbx_destroy(h); }
    };
    static HostHandle host;

    const cv::Mat &K1 = pKF1->mK;
    const cv::Mat &K2 = pKF2->mK;
    const cv::Mat R1w = pKF1->GetRotation();
    const cv::Mat t1w = pKF1->GetTranslation();
    const cv::Mat R2w = pKF2->GetRotation();
    const cv::Mat t2w = pKF2->GetTranslation();

    const int N = (int)vpMatches1.size();
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<size_t> vnIndexEdge;
    std::vector<float> x1c, x2c, obs1, obs2, w1, w2;
    for (int i = 0; i < N; i++) {
        if (!vpMatches1[i]) continue;
        MapPoint *pMP1 = vpMapPoints1[i];
        MapPoint *pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || !pMP2) continue;
        if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
        const cv::Mat P3D1w = pMP1->GetWorldPos();
        const cv::Mat P3D1c = R1w * P3D1w + t1w;
        const cv::Mat P3D2w = pMP2->GetWorldPos();
        const cv::Mat P3D2c = R2w * P3D2w + t2w;
        for (int c = 0; c < 3; c++) { x1c.push_back(P3D1c.at<float>(c)); x2c.push_back(P3D2c.at<float>(c)); }
        const cv::KeyPoint &kpUn1 = pKF1->mvKeysUn[i];
        const cv::KeyPoint &kpUn2 = pKF2->mvKeysUn[i2];
        obs1.push_back(kpUn1.pt.x); obs1.push_back(kpUn1.pt.y);
        obs2.push_back(kpUn2.pt.x); obs2.push_back(kpUn2.pt.y);
        w1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);
        w2.push_back(pKF2->mvInvLevelSigma2[kpUn2.octave]);
        vnIndexEdge.push_back((size_t)i);
    }
    const int nCorrespondences = (int)vnIndexEdge.size();
    if (nCorrespondences == 0) return 0;                  // optimize() has nothing to do, nBad == 0, 0 < 10

    std::vector<uint8_t> keep((size_t)nCorrespondences, 1);
    orbx_sim3opt_problem P;
    P.n = nCorrespondences;
    P.x1c = x1c.data(); P.x2c = x2c.data(); P.obs1 = obs1.data(); P.obs2 = obs2.data();
    P.inv_sigma2_1 = w1.data(); P.inv_sigma2_2 = w2.data();
    P.camera1[0] = K1.at<float>(0, 0); P.camera1[1] = K1.at<float>(1, 1); P.camera1[2] = K1.at<float>(0, 2); P.camera1[3] = K1.at<float>(1, 2);
    P.camera2[0] = K2.at<float>(0, 0); P.camera2[1] = K2.at<float>(1, 1); P.camera2[2] = K2.at<float>(0, 2); P.camera2[3] = K2.at<float>(1, 2);
    const Eigen::Matrix3d R = g2oS12.rotation().toRotationMatrix();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) P.R[3 * r + c] = (float)R(r, c);
        P.t[r] = (float)g2oS12.translation()[r];
    }
    P.s = (float)g2oS12.scale();
    P.th2 = th2;
    P.fix_scale = bFixScale ? 1 : 0;
    P.keep = keep.data();
    orbx_sim3opt_result res;
    if (orbx_optimize_sim3_batch(host.h, 1, &P, &res) != ORBX_OK) throw std::runtime_error(orbx_last_error());

    for (int j = 0; j < nCorrespondences; j++)
        if (!keep[j]) vpMatches1[vnIndexEdge[j]] = static_cast<MapPoint *>(NULL);
    if (!res.written) return 0;                           // fewer than 10 survived the first test: g2oS12 stays
    g2oS12 = g2o::Sim3(Eigen::Quaterniond(res.r[3], res.r[0], res.r[1], res.r[2]), Eigen::Vector3d(res.t[0], res.t[1], res.t[2]), res.s);
    return res.ninliers;
}
