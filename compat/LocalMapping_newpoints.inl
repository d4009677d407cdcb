// compat/LocalMapping_newpoints.inl -- the per-match loop of LocalMapping::CreateNewMapPoints for ONE neighbour keyframe
// (reference src/LocalMapping.cc:447-678, `for (int ikp = 0; ikp < nmatches; ikp++) { ... }`): marshal, ONE call of the library,
// the new MapPoints created in match order.
//
// How to apply (maintainer, inside the ORB-SLAM2 tree; needs OpenCV -- this repository's tests run the fragment against working
// stand-ins, tests/compat_newpoints/, and the maintainer's build remains the final check): include <stdexcept>, <vector>,
// <cstdint> and "orbx.h" at the top of src/LocalMapping.cc and, inside the neighbour loop of CreateNewMapPoints, replace the
// statement `const int nmatches = vMatchedIndices.size();` and the whole `for (int ikp ...)` loop after it by
//
//   #include "LocalMapping_newpoints.inl"
//
// The fragment is a block of statements.  It reads what the function holds at that place -- mpCurrentKeyFrame, pKF2,
// vMatchedIndices, Rcw1, tcw1, Ow1, Rcw2, tcw2, Ow2, mpMap -- and the keyframes' public members (fx .. invfy, mb, mbf, mvKeysUn,
// mvKeys, mvuRight, mvDepth, mvScaleFactors, mvLevelSigma2, mfScaleFactor), and for every accepted match, in match order, does what
// :655-677 does: the MapPoint, the two observations, AddMapPoint on both keyframes, ComputeDistinctiveDescriptors,
// UpdateNormalAndDepth, Map::AddMapPoint, mlpRecentAddedMapPoints, nnew.  Everything around it stays the reference's: the
// covisible neighbours, the baseline / median-depth gate, ComputeF12 and SearchForTriangulation (or compat/ORBmatcher.h's).
// Rwc1, Rwc2, Tcw1, Tcw2, ratioFactor and the fx1 .. invfy2 references of the function are no longer read.
//
// Which path a lone call takes follows profiles/newpoints_batch.md: measured on an MI355X, one problem per call takes
// 29 / 30 / 38 us on the device against 13 / 37 / 104 us on the library's host path for 30 / 100 / 300 matches, so a call with
// fewer than ORBX_NEWPOINTS_DEVICE_MIN = 100 matches runs the host path (a host-only handle) and every other call the device;
// both handles are thread_local and created at the first use (a handle is not re-entrant).  Define ORBX_LOCALMAPPING_HANDLE
// to an expression of type orbx_handle* to run every call on that handle instead (a host-only handle runs the library's host
// path); ORBX_NEWPOINTS=host in the environment, read per call, sends the call to the host path.  A mapper with many streams does
// not use this fragment: it collects one neighbour per stream and calls orbx_create_new_map_points_batch with all of them
// (INTEGRATION.md section 12).
//
// Statuses and points are the library's (one-sided Jacobi where the reference calls cv::SVD::compute,
// its own rules for cv::norm, Mat::dot, the products, atan2f and cosf); parity with an OpenCV build is not pinned.  A feature with
// mvuRight >= 0 and no positive mvDepth, where the reference dereferences an empty cv::Mat, is skipped.
{
#ifndef ORBX_NEWPOINTS_DEVICE_MIN
#define ORBX_NEWPOINTS_DEVICE_MIN 100
#endif
    const int orbx_n = (int)vMatchedIndices.size();
    if (orbx_n > 0) {
#ifdef ORBX_LOCALMAPPING_HANDLE
        orbx_handle *orbx_np_h = (ORBX_LOCALMAPPING_HANDLE);
#else
        struct OrbxNewPointsHolder {
            orbx_handle *h[2] = {NULL, NULL};                        // host path, device
            ~OrbxNewPointsHolder() { orbx_destroy(h[0]); orbx_destroy(h[1]); }
        };
        thread_local OrbxNewPointsHolder orbx_np_t;
        const int orbx_np_which = orbx_n < ORBX_NEWPOINTS_DEVICE_MIN ? 0 : 1;
        if (!orbx_np_t.h[orbx_np_which]) {
            orbx_params prm;
            orbx_default_params(&prm);
            if (orbx_np_which == 0) prm.device = -2;                 // host-only: the library's host path
            if (orbx_create(&prm, &orbx_np_t.h[orbx_np_which]) != ORBX_OK) throw std::runtime_error(orbx_last_error());
        }
        orbx_handle *orbx_np_h = orbx_np_t.h[orbx_np_which];
#endif
        static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint is the 28-byte record of OpenCV 2.4 / 3.x");
        KeyFrame *orbx_kf[2] = {mpCurrentKeyFrame, pKF2};
        const cv::Mat *orbx_pose[2][3] = {{&Rcw1, &tcw1, &Ow1}, {&Rcw2, &tcw2, &Ow2}};
        std::vector<float> orbx_keys[2];
        orbx_newpoints_problem orbx_P;
        orbx_newpoints_keyframe *orbx_view[2] = {&orbx_P.kf1, &orbx_P.kf2};
        for (int s = 0; s < 2; s++) {
            KeyFrame *kf = orbx_kf[s];
            orbx_newpoints_keyframe &V = *orbx_view[s];
            const size_t nf = kf->mvKeysUn.size();
            if (kf->mvKeys.size() != nf || kf->mvuRight.size() != nf || kf->mvDepth.size() != nf ||
                kf->mvLevelSigma2.size() != kf->mvScaleFactors.size())
                throw std::runtime_error("LocalMapping: a keyframe's feature arrays or scale tables differ in length");
            for (int i = 0; i < 9; i++) V.Rcw[i] = orbx_pose[s][0]->at<float>(i / 3, i % 3);
            for (int i = 0; i < 3; i++) { V.tcw[i] = orbx_pose[s][1]->at<float>(i); V.Ow[i] = orbx_pose[s][2]->at<float>(i); }
            V.fx = kf->fx; V.fy = kf->fy; V.cx = kf->cx; V.cy = kf->cy; V.invfx = kf->invfx; V.invfy = kf->invfy;
            V.mb = kf->mb; V.mbf = kf->mbf;
            V.nlevels = (int32_t)kf->mvScaleFactors.size();
            V.scale_factors = kf->mvScaleFactors.data(); V.level_sigma2 = kf->mvLevelSigma2.data();
            orbx_keys[s].resize(2 * nf);
            for (size_t i = 0; i < nf; i++) { orbx_keys[s][2 * i] = kf->mvKeys[i].pt.x; orbx_keys[s][2 * i + 1] = kf->mvKeys[i].pt.y; }
            V.n = (int32_t)nf;
            V.keys_un = reinterpret_cast<const orbx_keypoint *>(kf->mvKeysUn.data());
            V.keys = orbx_keys[s].data(); V.u_right = kf->mvuRight.data(); V.depth = kf->mvDepth.data();
        }
        std::vector<int32_t> orbx_m(2 * (size_t)orbx_n);
        for (int i = 0; i < orbx_n; i++) { orbx_m[2 * i] = (int32_t)vMatchedIndices[i].first; orbx_m[2 * i + 1] = (int32_t)vMatchedIndices[i].second; }
        orbx_P.scale_factor = mpCurrentKeyFrame->mfScaleFactor;
        orbx_P.nmatches = orbx_n; orbx_P.matches = orbx_m.data();
        std::vector<uint8_t> orbx_st((size_t)orbx_n);
        std::vector<float> orbx_pts(3 * (size_t)orbx_n);
        if (orbx_create_new_map_points_batch(orbx_np_h, 1, &orbx_P, orbx_st.data(), orbx_pts.data()) != ORBX_OK)
            throw std::runtime_error(orbx_last_error());
        for (int i = 0; i < orbx_n; i++) {
            if (orbx_st[i] > ORBX_NEWPOINT_STEREO2) continue;        // every rejecting status: the reference's `continue`
            const int idx1 = (int)vMatchedIndices[i].first, idx2 = (int)vMatchedIndices[i].second;
            cv::Mat x3D(3, 1, CV_32F);
            for (int c = 0; c < 3; c++) x3D.at<float>(c) = orbx_pts[3 * i + c];
            MapPoint *pMP = new MapPoint(x3D, mpCurrentKeyFrame, mpMap);
            pMP->AddObservation(mpCurrentKeyFrame, idx1);
            pMP->AddObservation(pKF2, idx2);
            mpCurrentKeyFrame->AddMapPoint(pMP, idx1);
            pKF2->AddMapPoint(pMP, idx2);
            pMP->ComputeDistinctiveDescriptors();
            pMP->UpdateNormalAndDepth();
            mpMap->AddMapPoint(pMP);
            mlpRecentAddedMapPoints.push_back(pMP);
            nnew++;
        }
    }
}
