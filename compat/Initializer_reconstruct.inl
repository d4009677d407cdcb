// compat/Initializer_reconstruct.inl -- the bodies of Initializer::ReconstructH and Initializer::ReconstructF (reference
// src/Initializer.cc:1154-1462 and :963-1132): marshal, ONE stand-alone call of the library, scatter.
//
// How to apply (maintainer, inside the ORB-SLAM2 tree; needs OpenCV -- this repository's tests run the fragment against working
// stand-ins, tests/compat_recon/, and the maintainer's build remains the final check): include <stdexcept>, <vector>, <cstdint>
// and "orbx.h" at the top of src/Initializer.cc and replace the two bodies by
//
//   bool Initializer::ReconstructH(vector<bool> &vbMatchesInliers, cv::Mat &H21, cv::Mat &K, cv::Mat &R21, cv::Mat &t21,
//                                  vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated, float minParallax, int minTriangulated)
//   {
//   #define ORBX_RECONSTRUCT_MODEL ORBX_INIT_H
//   #define ORBX_RECONSTRUCT_MATRIX H21
//   #include "Initializer_reconstruct.inl"
//   }
//
// and the same with ORBX_INIT_F and F21 for ReconstructF.  The fragment is a block of statements followed by the function's
// return statement; it undefines both macros.  It reads mvKeys1, mvKeys2, mvMatches12 and mSigma and the function's arguments,
// and leaves R21, t21, vP3D and vbTriangulated as the reference does: on success R21 (3 x 3) and t21 (3 x 1) CV_32F, vP3D and
// vbTriangulated of mvKeys1.size() entries, written per match in match order at vMatches12[i].first -- the point of a counted
// match, true where cosParallax < 0.99998, false again where a later match of the same keypoint gives a point that is not
// finite --; on failure R21 and t21 are the empty cv::Mat the reference resets them to (ReconstructF) or are left alone
// (ReconstructH), and vP3D and vbTriangulated are left alone.  DecomposeE, CheckRT and Triangulate are no longer called.
//
// Which path a lone call takes: the DEVICE, on a thread_local handle created on the current device at the first use (a handle is
// not re-entrant).  profiles/recon_batch.md has the measurement behind that default.  Define ORBX_INITIALIZER_HANDLE to an
// expression of type orbx_handle* to run on that handle instead (a host-only handle runs the library's host path);
// ORBX_RECON=host in the environment, read per call, sends the call to the host path.  A tracker with many streams does not use
// this fragment: it collects the outstanding attempts and calls orbx_initialize_batch_create or
// orbx_init_reconstruct_batch_create with all of them.
//
// The poses and points are the library's (one-sided Jacobi where the reference calls cv::SVD::compute,
// its own rules for cv::determinant, cv::norm, Mat::dot and the products, the order statistic by value); parity with an OpenCV
// build is not pinned.
#ifdef ORBX_INITIALIZER_HANDLE
    orbx_handle *orbx_rc_h = (ORBX_INITIALIZER_HANDLE);
#else
    struct OrbxReconHolder { orbx_handle *h = NULL; ~OrbxReconHolder() { orbx_destroy(h); } };
    thread_local OrbxReconHolder orbx_rc_t;
    if (!orbx_rc_t.h) {
        orbx_params prm;
        orbx_default_params(&prm);
        if (orbx_create(&prm, &orbx_rc_t.h) != ORBX_OK) throw std::runtime_error(orbx_last_error());
    }
    orbx_handle *orbx_rc_h = orbx_rc_t.h;
#endif
    const int orbx_N = (int)mvMatches12.size();
    if ((int)vbMatchesInliers.size() != orbx_N) throw std::runtime_error("Initializer: vbMatchesInliers does not have one entry per match");
    std::vector<float> orbx_k1(2 * mvKeys1.size()), orbx_k2(2 * mvKeys2.size());
    for (size_t i = 0; i < mvKeys1.size(); i++) { orbx_k1[2 * i] = mvKeys1[i].pt.x; orbx_k1[2 * i + 1] = mvKeys1[i].pt.y; }
    for (size_t i = 0; i < mvKeys2.size(); i++) { orbx_k2[2 * i] = mvKeys2[i].pt.x; orbx_k2[2 * i + 1] = mvKeys2[i].pt.y; }
    std::vector<int32_t> orbx_m(2 * (size_t)orbx_N);
    std::vector<uint8_t> orbx_inl((size_t)orbx_N + 1), orbx_st((size_t)orbx_N + 1);
    std::vector<float> orbx_pts(3 * (size_t)orbx_N + 3);
    for (int i = 0; i < orbx_N; i++) {
        orbx_m[2 * i] = (int32_t)mvMatches12[i].first; orbx_m[2 * i + 1] = (int32_t)mvMatches12[i].second;
        orbx_inl[i] = vbMatchesInliers[i] ? 1 : 0;
    }
    orbx_recon_problem orbx_P;
    orbx_P.n1 = (int32_t)mvKeys1.size(); orbx_P.n2 = (int32_t)mvKeys2.size();
    orbx_P.keys1 = orbx_k1.empty() ? NULL : orbx_k1.data(); orbx_P.keys2 = orbx_k2.empty() ? NULL : orbx_k2.data();
    orbx_P.n = orbx_N; orbx_P.matches = orbx_m.empty() ? NULL : orbx_m.data(); orbx_P.inliers = orbx_inl.data();
    orbx_P.model = ORBX_RECONSTRUCT_MODEL;
    for (int i = 0; i < 9; i++) orbx_P.M[i] = (ORBX_RECONSTRUCT_MATRIX).at<float>(i / 3, i % 3);
    orbx_P.K[0] = K.at<float>(0, 0); orbx_P.K[1] = K.at<float>(1, 1); orbx_P.K[2] = K.at<float>(0, 2); orbx_P.K[3] = K.at<float>(1, 2);
    orbx_P.sigma = mSigma; orbx_P.min_parallax = minParallax; orbx_P.min_triangulated = minTriangulated;
    orbx_recon_batch *orbx_b = NULL;
    if (orbx_init_reconstruct_batch_create(orbx_rc_h, 1, &orbx_P, &orbx_b) != ORBX_OK) throw std::runtime_error(orbx_last_error());
    int32_t orbx_ok = 0;
    float orbx_R9[9], orbx_t3[3];
    const orbx_status orbx_st_rc = orbx_recon_batch_result(orbx_b, 0, &orbx_ok, orbx_R9, orbx_t3, NULL, orbx_st.data(), orbx_pts.data(), NULL);
    orbx_recon_batch_destroy(orbx_b);
    if (orbx_st_rc != ORBX_OK) throw std::runtime_error(orbx_last_error());
    if (ORBX_RECONSTRUCT_MODEL == ORBX_INIT_F) { R21 = cv::Mat(); t21 = cv::Mat(); }     // :1042-1043, before every return but the first
    if (orbx_ok) {
        vP3D = std::vector<cv::Point3f>(mvKeys1.size());
        vbTriangulated = std::vector<bool>(mvKeys1.size(), false);
        for (int i = 0; i < orbx_N; i++) {
            const size_t orbx_first = (size_t)mvMatches12[i].first;
            if (orbx_st[i] == 1) vbTriangulated[orbx_first] = false;
            else if (orbx_st[i] >= 2) {
                vP3D[orbx_first] = cv::Point3f(orbx_pts[3 * i], orbx_pts[3 * i + 1], orbx_pts[3 * i + 2]);
                if (orbx_st[i] == 3) vbTriangulated[orbx_first] = true;
            }
        }
        R21 = cv::Mat(3, 3, CV_32F);
        t21 = cv::Mat(3, 1, CV_32F);
        for (int i = 0; i < 9; i++) R21.at<float>(i / 3, i % 3) = orbx_R9[i];
        for (int i = 0; i < 3; i++) t21.at<float>(i, 0) = orbx_t3[i];
    }
#undef ORBX_RECONSTRUCT_MODEL
#undef ORBX_RECONSTRUCT_MATRIX
    return orbx_ok != 0;
