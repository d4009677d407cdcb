// compat/Sim3Solver.h -- drop-in replacement of the reference's include/Sim3Solver.h + src/Sim3Solver.cc.
//
// Same namespace, class name and public surface (the constructor, SetRansacParameters, find, iterate, GetEstimatedRotation /
// Translation / Scale), so LoopClosing::ComputeSim3 (src/LoopClosing.cc:425-577) compiles unchanged.  The RANSAC itself -- every
// ComputeSim3 + CheckInliers of every solver -- runs in liborbx.so (include/orbx.h: orbx_sim3_ransac_batch_create) and
// iterate() is the library's cursor over the stored results.
//
// One addition: the static Sim3Solver::Prepare(std::vector<Sim3Solver*>&) issues ONE batch call for all solvers of a
// ComputeSim3 loop (NULL entries, the discarded candidates, are skipped); call it between the loop that creates the solvers
// and the while loop that iterates them.  A solver that was not prepared runs alone with its first iterate().
// Sim3Solver::SetHandle(extractor->handle()) shares the extractor's handle (device, stream, staging block); without it the
// first use creates a handle on the current device.
//
// What stays here is what the constructor does in the reference (:84-133), restated: a correspondence is kept when both
// MapPoints exist, neither is bad and both have an index in their keyframe; its camera-frame points are Rcw * Xw + tcw through
// cv::Mat (OpenCV's arithmetic, as in the reference), its thresholds 9.210 * mvLevelSigma2[octave] formed in double and stored
// as float, and mvnIndices1 maps the solver's inlier flags back to the slots of vpMatched12.
//
// ONE deviation: the reference draws a triple from DUtils::Random::RandomInt inside iterate(), lazily, and
// stops drawing when it returns; this class draws all mRansacMaxIts triples of a solver when it is prepared.  The global
// rand() stream is therefore consumed in another order than in the reference; each solver's answer is the reference's for the
// draws it was given.  Parity of the arithmetic with an OpenCV build is not pinned from N to R.
// A solver with fewer than 3 correspondences never draws (the reference's RandomInt(0, -1) is undefined there) and reports
// bNoMore at once.  SetRansacParameters discards a preparation and restarts the solver, so call it before Prepare, as
// ComputeSim3 does.
//
// Needs the ORB-SLAM2 tree (KeyFrame.h, MapPoint.h, Thirdparty/DBoW2/DUtils/Random.h).  This repository's tests build and run
// it against stand-ins of those (tests/compat_sim3/); the maintainer's build inside an ORB-SLAM2 tree remains
// the final check.  Remove src/Sim3Solver.cc from the library's sources.
#ifndef SIM3SOLVER_H
#define SIM3SOLVER_H

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "orbx.h"

namespace ORB_SLAM2 {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale = true)
        : mN1((int)vpMatched12.size()), mbFixScale(bFixScale) {
        const std::vector<MapPoint *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        const cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation();
        const cv::Mat Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
        for (int i1 = 0; i1 < mN1; i1++) {
            MapPoint *pMP2 = vpMatched12[i1];
            if (!pMP2) continue;
            MapPoint *pMP1 = vpKeyFrameMP1[i1];
            if (!pMP1 || pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            const float sigmaSquare1 = pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave];
            const float sigmaSquare2 = pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave];
            mvnMaxError1.push_back(9.210 * sigmaSquare1);
            mvnMaxError2.push_back(9.210 * sigmaSquare2);
            mvnIndices1.push_back((size_t)i1);
            const cv::Mat X1 = Rcw1 * pMP1->GetWorldPos() + tcw1, X2 = Rcw2 * pMP2->GetWorldPos() + tcw2;
            for (int c = 0; c < 3; c++) { mvX3Dc1.push_back(X1.at<float>(c)); mvX3Dc2.push_back(X2.at<float>(c)); }
        }
        N = (int)mvnIndices1.size();
        const cv::Mat K1 = pKF1->mK, K2 = pKF2->mK;
        mK1[0] = K1.at<float>(0, 0); mK1[1] = K1.at<float>(1, 1); mK1[2] = K1.at<float>(0, 2); mK1[3] = K1.at<float>(1, 2);
        mK2[0] = K2.at<float>(0, 0); mK2[1] = K2.at<float>(1, 1); mK2[2] = K2.at<float>(0, 2); mK2[3] = K2.at<float>(1, 2);
        SetRansacParameters();
    }
    Sim3Solver(const Sim3Solver &) = delete;
    Sim3Solver &operator=(const Sim3Solver &) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = orbx_sim3_ransac_iterations(N, probability, minInliers, maxIterations);
        batch_.reset();
        k_ = -1;
    }

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
        if (!batch_) {
            std::vector<Sim3Solver *> one(1, this);
            Prepare(one);
        }
        vbInliers = std::vector<bool>((size_t)mN1, false);
        std::vector<uint8_t> flags((size_t)(N > 0 ? N : 1), 0);
        int32_t no_more = 0, n = 0;
        float T[16];
        const int32_t r = orbx_sim3_batch_iterate(batch_->b, k_, nIterations, &no_more, flags.data(), &n, T);
        if (r < 0) throw std::runtime_error(std::string("Sim3Solver::iterate: ") + orbx_last_error());
        bNoMore = no_more != 0;
        nInliers = n;
        if (r == 0) return cv::Mat();
        for (int i = 0; i < N; i++)
            if (flags[i]) vbInliers[mvnIndices1[i]] = true;
        cv::Mat T12(4, 4, CV_32F);
        for (int i = 0; i < 16; i++) T12.at<float>(i / 4, i % 4) = T[i];
        return T12;
    }

    cv::Mat GetEstimatedRotation() {
        float R[9], t[3], s;
        if (!Best(R, t, &s)) return cv::Mat();
        cv::Mat m(3, 3, CV_32F);
        for (int i = 0; i < 9; i++) m.at<float>(i / 3, i % 3) = R[i];
        return m;
    }
    cv::Mat GetEstimatedTranslation() {
        float R[9], t[3], s;
        if (!Best(R, t, &s)) return cv::Mat();
        cv::Mat m(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) m.at<float>(i) = t[i];
        return m;
    }
    float GetEstimatedScale() {
        float R[9], t[3], s = 0.f;
        Best(R, t, &s);
        return s;
    }

    // not in the reference --------------------------------------------------------------------------------------------
    static void SetHandle(orbx_handle *h) { Shared().h = h; }
    // One batch call for every non-NULL solver of the list: draws each solver's triples (in list order), uploads, runs, and
    // points every solver at its slot of the result.  A solver prepared before starts again from its first iteration.
    static void Prepare(std::vector<Sim3Solver *> &solvers) {
        std::vector<Sim3Solver *> live;
        for (size_t i = 0; i < solvers.size(); i++)
            if (solvers[i]) live.push_back(solvers[i]);
        if (live.empty()) return;
        std::vector<orbx_sim3_problem> probs(live.size());
        for (size_t k = 0; k < live.size(); k++) {
            Sim3Solver &S = *live[k];
            orbx_sim3_problem &P = probs[k];
            S.Draw();
            P.n = S.N >= 3 ? S.N : 0;                      // fewer than 3 correspondences: nothing can be drawn, "no more" at once
            P.x1c = P.n ? S.mvX3Dc1.data() : NULL; P.x2c = P.n ? S.mvX3Dc2.data() : NULL;
            P.max_err1 = P.n ? S.mvnMaxError1.data() : NULL; P.max_err2 = P.n ? S.mvnMaxError2.data() : NULL;
            for (int c = 0; c < 4; c++) { P.camera1[c] = S.mK1[c]; P.camera2[c] = S.mK2[c]; }
            P.fix_scale = S.mbFixScale ? 1 : 0;
            P.min_inliers = S.N >= 3 ? S.mRansacMinInliers : (S.mRansacMinInliers > 1 ? S.mRansacMinInliers : 1);
            P.iterations = S.mRansacMaxIts;
            P.sets = S.sets_.empty() ? NULL : S.sets_.data();
        }
        std::shared_ptr<Batch> b = std::make_shared<Batch>();
        if (orbx_sim3_ransac_batch_create(Handle(), (int)probs.size(), probs.data(), &b->b) != ORBX_OK)
            throw std::runtime_error(std::string("Sim3Solver::Prepare: ") + orbx_last_error());
        for (size_t k = 0; k < live.size(); k++) { live[k]->batch_ = b; live[k]->k_ = (int)k; }
    }
    const std::vector<int32_t> &Draws() const { return sets_; }   // the triples of the last preparation, [mRansacMaxIts][3]
    int Correspondences() const { return N; }
    int MaxIterations() const { return mRansacMaxIts; }

private:
    struct Batch {
        orbx_sim3_batch *b = NULL;
        ~Batch() { orbx_sim3_batch_destroy(b); }
    };
    struct SharedState {
        orbx_handle *h = NULL, *own = NULL;
        ~SharedState() { if (own) orbx_destroy(own); }
    };
    static SharedState &Shared() { static SharedState s; return s; }
    static orbx_handle *Handle() {
        SharedState &s = Shared();
        if (s.h) return s.h;
        if (!s.own) {
            orbx_params p;
            orbx_default_params(&p);
            if (orbx_create(&p, &s.own) != ORBX_OK) throw std::runtime_error(std::string("Sim3Solver: ") + orbx_last_error());
        }
        return s.own;
    }
    // the draws of iterate() (:237-258), all iterations at once: three indices without replacement from a list that shrinks
    // by moving its last entry into the drawn position
    void Draw() {
        sets_.clear();
        if (N < 3 || N < mRansacMinInliers) return;
        std::vector<int32_t> all((size_t)N), avail;
        for (int i = 0; i < N; i++) all[i] = i;
        for (int it = 0; it < mRansacMaxIts; it++) {
            avail = all;
            for (int c = 0; c < 3; c++) {
                const int r = DUtils::Random::RandomInt(0, (int)avail.size() - 1);
                sets_.push_back(avail[r]);
                avail[r] = avail.back();
                avail.pop_back();
            }
        }
    }
    bool Best(float *R, float *t, float *s) { return batch_ && orbx_sim3_batch_best(batch_->b, k_, R, t, s) == ORBX_OK; }

    int mN1, N = 0;
    bool mbFixScale;
    std::vector<float> mvX3Dc1, mvX3Dc2, mvnMaxError1, mvnMaxError2;
    std::vector<size_t> mvnIndices1;
    float mK1[4], mK2[4];
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300;
    std::vector<int32_t> sets_;
    std::shared_ptr<Batch> batch_;
    int k_ = -1;
};

}  // namespace ORB_SLAM2

#endif  // SIM3SOLVER_H
