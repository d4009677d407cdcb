// compat/PnPsolver.h -- drop-in replacement of the reference's include/PnPsolver.h + src/PnPsolver.cc.
//
// Same namespace, class name and public surface (the constructor, SetRansacParameters, find, iterate), so
// Tracking::Relocalization (src/Tracking.cc:2240-2500) compiles unchanged.  The RANSAC itself -- every 4-point EPnP and every
// CheckInliers of every solver -- runs in liborbx.so (include/orbx.h: orbx_pnp_ransac_batch_create) and iterate() is the
// library's cursor over the stored results, Refine() included.
//
// One addition: the static PnPsolver::Prepare(std::vector<PnPsolver*>&) issues ONE batch call for all solvers of a
// Relocalization (NULL entries, the discarded candidates, are skipped); call it between the loop that creates the solvers and
// the while loop that iterates them.  A solver that was not prepared runs alone with its first iterate().
// PnPsolver::SetHandle(extractor->handle()) shares the extractor's handle (device, stream, staging block); without it the first
// use creates a handle on the current device.
//
// What stays here is what the constructor does in the reference (:120-168), restated: a correspondence is kept when its MapPoint
// exists and is not bad; mvP2D is mvKeysUn[i].pt, mvSigma2 is mvLevelSigma2[octave], mvP3Dw the float world position,
// mvKeyPointIndices maps the solver's inlier flags back to the slots of vpMapPointMatches; fu, fv, uc, vc are doubles.
// SetRansacParameters is orbx_pnp_ransac_parameters plus mvMaxError[i] = mvSigma2[i] * th2 (a float times a float).
//
// ONE deviation: the reference draws four indices from DUtils::Random::RandomInt inside iterate(), lazily,
// and stops drawing when it returns; this class draws all mRansacMaxIts sets of a solver when it is prepared, and when a call
// needs an iteration past those (the loop condition of :285 is an OR, and a solver may be iterated again after
// PoseOptimization rejected its answer) it draws one more set at a time, appends it (orbx_pnp_batch_append) and repeats the
// call.  The global rand() stream is therefore consumed in another order than in the reference; each solver's answer is the
// reference's for the draws it was given.  Parity of the arithmetic with an OpenCV build is not pinned (DESIGN.md section 2,
// F13).  SetRansacParameters discards a preparation and restarts the solver, so call it before Prepare, as Relocalization does.
//
// Needs the ORB-SLAM2 tree (Frame.h, MapPoint.h, Thirdparty/DBoW2/DUtils/Random.h).  This repository's tests build and run it
// against stand-ins of those (tests/compat_pnp/); the maintainer's build inside an ORB-SLAM2 tree remains the
// final check.  Remove src/PnPsolver.cc from the library's sources.
#ifndef PNPSOLVER_H
#define PNPSOLVER_H

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "Frame.h"
#include "MapPoint.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "orbx.h"

namespace ORB_SLAM2 {

class PnPsolver {
public:
    PnPsolver(const Frame &F, const std::vector<MapPoint *> &vpMapPointMatches) : mnSlots(vpMapPointMatches.size()) {
        for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
            MapPoint *pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) continue;
            const cv::KeyPoint &kp = F.mvKeysUn[i];
            mvP2D.push_back(kp.pt.x); mvP2D.push_back(kp.pt.y);
            mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
            const cv::Mat Pos = pMP->GetWorldPos();
            for (int c = 0; c < 3; c++) mvP3Dw.push_back(Pos.at<float>(c));
            mvKeyPointIndices.push_back(i);
        }
        N = (int)mvKeyPointIndices.size();
        mCamera[0] = F.fx; mCamera[1] = F.fy; mCamera[2] = F.cx; mCamera[3] = F.cy;
        SetRansacParameters();
    }
    PnPsolver(const PnPsolver &) = delete;
    PnPsolver &operator=(const PnPsolver &) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                             float th2 = 5.991) {
        if (minSet != 4) throw std::runtime_error("PnPsolver: the batched solver draws minimal sets of 4");
        int32_t mi = 0, its = 0;
        orbx_pnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mi, &its);
        mRansacMinInliers = mi;
        mRansacMaxIts = its;
        mvMaxError.resize(mvSigma2.size());
        for (size_t i = 0; i < mvSigma2.size(); i++) mvMaxError[i] = mvSigma2[i] * th2;
        batch_.reset();
        k_ = -1;
    }

    cv::Mat find(std::vector<bool> &vbInliers, int &nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
    }

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
        if (!batch_) {
            std::vector<PnPsolver *> one(1, this);
            Prepare(one);
        }
        vbInliers.clear();
        std::vector<uint8_t> flags((size_t)(N > 0 ? N : 1), 0);
        int32_t no_more = 0, n = 0, r;
        float T[16];
        for (;;) {
            r = orbx_pnp_batch_iterate(batch_->b, k_, nIterations, &no_more, flags.data(), &n, T);
            if (r != -2) break;
            int32_t set[4];                                    // the call needs an iteration that was not drawn: draw it now
            DrawOne(set);
            sets_.insert(sets_.end(), set, set + 4);
            if (orbx_pnp_batch_append(batch_->b, k_, 1, set) != ORBX_OK)
                throw std::runtime_error(std::string("PnPsolver::iterate: ") + orbx_last_error());
        }
        if (r < 0) throw std::runtime_error(std::string("PnPsolver::iterate: ") + orbx_last_error());
        bNoMore = no_more != 0;
        nInliers = n;
        if (r == 0) return cv::Mat();
        vbInliers = std::vector<bool>(mnSlots, false);
        for (int i = 0; i < N; i++)
            if (flags[i]) vbInliers[mvKeyPointIndices[i]] = true;
        cv::Mat Tcw(4, 4, CV_32F);
        for (int i = 0; i < 16; i++) Tcw.at<float>(i / 4, i % 4) = T[i];
        return Tcw;
    }

    // not in the reference --------------------------------------------------------------------------------------------
    static void SetHandle(orbx_handle *h) { Shared().h = h; }
    // One batch call for every non-NULL solver of the list: draws each solver's mRansacMaxIts sets (in list order), uploads,
    // runs, and points every solver at its slot of the result.  A solver prepared before starts again from its first iteration.
    static void Prepare(std::vector<PnPsolver *> &solvers) {
        std::vector<PnPsolver *> live;
        for (size_t i = 0; i < solvers.size(); i++)
            if (solvers[i]) live.push_back(solvers[i]);
        if (live.empty()) return;
        std::vector<orbx_pnp_problem> probs(live.size());
        for (size_t k = 0; k < live.size(); k++) {
            PnPsolver &S = *live[k];
            orbx_pnp_problem &P = probs[k];
            S.Draw();
            P.n = S.N;
            P.p3dw = S.N ? S.mvP3Dw.data() : NULL;
            P.p2d = S.N ? S.mvP2D.data() : NULL;
            P.max_err = S.N ? S.mvMaxError.data() : NULL;
            for (int c = 0; c < 4; c++) P.camera[c] = S.mCamera[c];
            P.min_inliers = S.mRansacMinInliers;
            P.iterations = S.mRansacMaxIts;
            P.sets = S.sets_.empty() ? NULL : S.sets_.data();
        }
        std::shared_ptr<Batch> b = std::make_shared<Batch>();
        if (orbx_pnp_ransac_batch_create(Handle(), (int)probs.size(), probs.data(), &b->b) != ORBX_OK)
            throw std::runtime_error(std::string("PnPsolver::Prepare: ") + orbx_last_error());
        for (size_t k = 0; k < live.size(); k++) { live[k]->batch_ = b; live[k]->k_ = (int)k; }
    }
    const std::vector<int32_t> &Draws() const { return sets_; }   // every set drawn since the last preparation, [.][4]
    int Correspondences() const { return N; }
    int MinInliers() const { return mRansacMinInliers; }
    int MaxIterations() const { return mRansacMaxIts; }
    const std::vector<size_t> &KeyPointIndices() const { return mvKeyPointIndices; }

private:
    struct Batch {
        orbx_pnp_batch *b = NULL;
        ~Batch() { orbx_pnp_batch_destroy(b); }
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
            if (orbx_create(&p, &s.own) != ORBX_OK) throw std::runtime_error(std::string("PnPsolver: ") + orbx_last_error());
        }
        return s.own;
    }
    // the draw of one iteration (:293-310): four indices without replacement from a list that shrinks by moving its last entry
    // into the drawn position
    void DrawOne(int32_t *set) {
        std::vector<int32_t> avail((size_t)N);
        for (int i = 0; i < N; i++) avail[i] = i;
        for (int c = 0; c < 4; c++) {
            const int r = DUtils::Random::RandomInt(0, (int)avail.size() - 1);
            set[c] = avail[r];
            avail[r] = avail.back();
            avail.pop_back();
        }
    }
    void Draw() {
        sets_.clear();
        if (N < mRansacMinInliers) return;                     // (mRansacMinInliers >= minSet = 4, so N >= 4 below)
        for (int it = 0; it < mRansacMaxIts; it++) {
            int32_t set[4];
            DrawOne(set);
            sets_.insert(sets_.end(), set, set + 4);
        }
    }

    size_t mnSlots;
    int N = 0;
    std::vector<float> mvP2D, mvSigma2, mvP3Dw, mvMaxError;
    std::vector<size_t> mvKeyPointIndices;
    double mCamera[4];
    int mRansacMinInliers = 8, mRansacMaxIts = 300;
    std::vector<int32_t> sets_;
    std::shared_ptr<Batch> batch_;
    int k_ = -1;
};

}  // namespace ORB_SLAM2

#endif  // PNPSOLVER_H
