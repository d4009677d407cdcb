// compat/Initializer_ransac.inl -- replacement for the two `thread` lines of Initializer::Initialize and their joins
// (reference src/Initializer.cc:204-215):
//
//     thread threadH(&Initializer::FindHomography, this, ref(vbMatchesInliersH), ref(SH), ref(H));
//     thread threadF(&Initializer::FindFundamental, this, ref(vbMatchesInliersF), ref(SF), ref(F));
//     threadH.join();
//     threadF.join();
//
// How to apply (maintainer, inside the ORB-SLAM2 tree; needs OpenCV -- this repository's tests run the fragment against working
// stand-ins, tests/compat_init/, and the maintainer's build remains the final check): include <stdexcept>, <vector>, <cstdint>
// and "orbx.h" at the top of src/Initializer.cc and put
//   #include "Initializer_ransac.inl"
// in place of those four statements.  The fragment is a block of statements.  It reads mvKeys1, mvKeys2, mvMatches12, mvSets,
// mSigma and mMaxIterations and fills vbMatchesInliersH, SH, H, vbMatchesInliersF, SF, F exactly as the two threads do: the best
// iteration of each model is the first strict maximum of its score from 0; when no iteration of a model scores above 0 its
// matrix stays the empty cv::Mat it was, its mask is all false and its score 0.  What follows in Initialize -- RH, the choice of
// the model, the calls of ReconstructH / ReconstructF -- stays the reference's text; the BODIES of ReconstructH and
// ReconstructF have a drop-in of their own, compat/Initializer_reconstruct.inl (with it DecomposeE, CheckRT and Triangulate are
// no longer called either).  Pinned: the six variables equal tests/init_model.py bit for bit for the same draws.  Not pinned:
// parity with an OpenCV build.  FindHomography, FindFundamental, ComputeH21, ComputeF21, CheckHomography, CheckFundamental and
// Normalize are no longer called from Initialize.
//
// ONE call evaluates both models: every iteration of H and of F is a lane of the same launch (include/orbx.h,
// orbx_init_ransac_batch_create).  The handle is thread_local, since a handle is not re-entrant, and is created on the current
// device at the first use; define ORBX_INITIALIZER_HANDLE to an expression of type orbx_handle* (the extractor's handle, say) to
// run on that one instead.  ORBX_INIT=host in the environment, read per call, sends the call to the library's host path.  A
// tracker with many streams does not use this fragment: it collects the outstanding attempts and calls
// orbx_init_ransac_batch_create with all of them.
//
// The matrices are the library's (one-sided Jacobi where the reference calls cv::SVDecomp); parity
// with an OpenCV build is not pinned.
{
#ifdef ORBX_INITIALIZER_HANDLE
    orbx_handle *orbx_init_h = (ORBX_INITIALIZER_HANDLE);
#else
    struct OrbxInitHolder { orbx_handle *h = NULL; ~OrbxInitHolder() { orbx_destroy(h); } };
    thread_local OrbxInitHolder orbx_init_t;
    if (!orbx_init_t.h) {
        orbx_params prm;
        orbx_default_params(&prm);
        if (orbx_create(&prm, &orbx_init_t.h) != ORBX_OK) throw std::runtime_error(orbx_last_error());
    }
    orbx_handle *orbx_init_h = orbx_init_t.h;
#endif
    const int orbx_N = (int)mvMatches12.size();
    std::vector<float> orbx_k1(2 * mvKeys1.size()), orbx_k2(2 * mvKeys2.size());
    for (size_t i = 0; i < mvKeys1.size(); i++) { orbx_k1[2 * i] = mvKeys1[i].pt.x; orbx_k1[2 * i + 1] = mvKeys1[i].pt.y; }
    for (size_t i = 0; i < mvKeys2.size(); i++) { orbx_k2[2 * i] = mvKeys2[i].pt.x; orbx_k2[2 * i + 1] = mvKeys2[i].pt.y; }
    std::vector<int32_t> orbx_m(2 * (size_t)orbx_N), orbx_sets(8 * mvSets.size());
    for (int i = 0; i < orbx_N; i++) { orbx_m[2 * i] = (int32_t)mvMatches12[i].first; orbx_m[2 * i + 1] = (int32_t)mvMatches12[i].second; }
    for (size_t it = 0; it < mvSets.size(); it++)
        for (size_t j = 0; j < 8; j++) orbx_sets[8 * it + j] = (int32_t)mvSets[it][j];
    orbx_init_problem orbx_P;
    orbx_P.n1 = (int32_t)mvKeys1.size(); orbx_P.n2 = (int32_t)mvKeys2.size();
    orbx_P.keys1 = orbx_k1.empty() ? NULL : orbx_k1.data(); orbx_P.keys2 = orbx_k2.empty() ? NULL : orbx_k2.data();
    orbx_P.n = orbx_N; orbx_P.matches = orbx_m.empty() ? NULL : orbx_m.data();
    orbx_P.sigma = mSigma; orbx_P.iterations = mMaxIterations;
    orbx_P.sets = orbx_sets.empty() ? NULL : orbx_sets.data();
    orbx_P.models = ORBX_INIT_H | ORBX_INIT_F;
    if ((int)mvSets.size() != mMaxIterations) throw std::runtime_error("Initializer: mvSets does not hold mMaxIterations sets");
    orbx_init_batch *orbx_b = NULL;
    if (orbx_init_ransac_batch_create(orbx_init_h, 1, &orbx_P, &orbx_b) != ORBX_OK) throw std::runtime_error(orbx_last_error());
    std::vector<uint8_t> orbx_iH((size_t)orbx_N + 1), orbx_iF((size_t)orbx_N + 1);
    float orbx_H9[9], orbx_F9[9];
    int32_t orbx_itH = -1, orbx_itF = -1;
    const orbx_status orbx_st = orbx_init_batch_result(orbx_b, 0, &SH, &SF, orbx_H9, orbx_F9, orbx_iH.data(), orbx_iF.data(), &orbx_itH,
                                                       &orbx_itF, NULL, NULL);
    orbx_init_batch_destroy(orbx_b);
    if (orbx_st != ORBX_OK) throw std::runtime_error(orbx_last_error());
    vbMatchesInliersH = std::vector<bool>(orbx_N, false);
    vbMatchesInliersF = std::vector<bool>(orbx_N, false);
    for (int i = 0; i < orbx_N; i++) { vbMatchesInliersH[i] = orbx_iH[i] != 0; vbMatchesInliersF[i] = orbx_iF[i] != 0; }
    if (orbx_itH >= 0) {
        H = cv::Mat(3, 3, CV_32F);
        for (int i = 0; i < 9; i++) H.at<float>(i / 3, i % 3) = orbx_H9[i];
    }
    if (orbx_itF >= 0) {
        F = cv::Mat(3, 3, CV_32F);
        for (int i = 0; i < 9; i++) F.at<float>(i / 3, i % 3) = orbx_F9[i];
    }
}
