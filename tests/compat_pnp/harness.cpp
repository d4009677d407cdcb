// tests/compat_pnp: one extern "C" entry point around compat/PnPsolver.h.  It builds one Frame (nslots keypoints) and K match
// vectors from flat arrays, one PnPsolver per candidate with Relocalization's SetRansacParameters call, optionally
// PnPsolver::Prepare, then plays ncalls iterate(call_n) calls on solver call_k and returns what each gave.  Every C++ exception
// is caught: -1 and cp_error().
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "PnPsolver.h"

using namespace ORB_SLAM2;
float Frame::fx = 0.f, Frame::fy = 0.f, Frame::cx = 0.f, Frame::cy = 0.f;
static std::string g_error;
extern "C" const char *cp_error() { return g_error.c_str(); }

static cv::Mat vec3(const float *p) {
    cv::Mat m(3, 1, CV_32F);
    for (int i = 0; i < 3; ++i) m.at<float>(i) = p[i];
    return m;
}

// state [K][nslots]: 0 = a sound point, 1 = NULL, 2 = bad.  inl_size [ncalls] = vbInliers.size() after the call.
extern "C" int cp_run(void *handle, int K, int nslots, const uint8_t *state, const float *pos, const float *kp, const int32_t *oct,
                      const float *camera4, double probability, int min_inliers, int max_iterations, float epsilon, uint64_t seed,
                      int prepare, int ncalls, const int32_t *call_k, const int32_t *call_n, int32_t *ret, int32_t *no_more,
                      int32_t *ninliers, float *Tcw, uint8_t *inliers, int32_t *inl_size, int32_t *solver_n, int32_t *solver_min,
                      int32_t *solver_its, int32_t *kp_index, int draw_cap, int32_t *draws, int32_t *ndraws) {
    try {
        PnPsolver::SetHandle((orbx_handle *)handle);
        DUtils::Random::State() = seed;
        Frame::fx = camera4[0]; Frame::fy = camera4[1]; Frame::cx = camera4[2]; Frame::cy = camera4[3];
        Frame F(8, 1.2f);
        F.mvKeysUn.resize((size_t)nslots);
        F.mvpMapPoints.assign((size_t)nslots, static_cast<MapPoint *>(NULL));
        for (int i = 0; i < nslots; ++i) { F.mvKeysUn[i].pt.x = kp[2 * i]; F.mvKeysUn[i].pt.y = kp[2 * i + 1]; F.mvKeysUn[i].octave = oct[i]; }
        std::vector<std::unique_ptr<MapPoint>> points;
        std::vector<std::unique_ptr<PnPsolver>> solvers;
        std::vector<PnPsolver *> list;
        for (int k = 0; k < K; ++k) {
            std::vector<MapPoint *> matches((size_t)nslots, static_cast<MapPoint *>(NULL));
            for (int i = 0; i < nslots; ++i) {
                const size_t e = (size_t)k * nslots + i;
                if (state[e] == 1) continue;
                points.emplace_back(new MapPoint(vec3(pos + 3 * e), state[e] == 2));
                matches[i] = points.back().get();
            }
            solvers.emplace_back(new PnPsolver(F, matches));
            solvers.back()->SetRansacParameters(probability, min_inliers, max_iterations, 4, epsilon, 5.991);
            list.push_back(solvers.back().get());
        }
        if (prepare) PnPsolver::Prepare(list);
        for (int c = 0; c < ncalls; ++c) {
            PnPsolver &S = *solvers[call_k[c]];
            bool bNoMore = false;
            std::vector<bool> vbInliers(3, true);              // iterate() clears it
            int nInliers = -1;
            const cv::Mat T = S.iterate(call_n[c], bNoMore, vbInliers, nInliers);
            ret[c] = T.empty() ? 0 : 1;
            no_more[c] = bNoMore ? 1 : 0;
            ninliers[c] = nInliers;
            inl_size[c] = (int32_t)vbInliers.size();
            if (!vbInliers.empty() && (int)vbInliers.size() != nslots) throw std::runtime_error("vbInliers has neither 0 nor nslots entries");
            for (size_t i = 0; i < vbInliers.size(); ++i) inliers[(size_t)c * nslots + i] = vbInliers[i] ? 1 : 0;
            if (!T.empty())
                for (int i = 0; i < 16; ++i) Tcw[16 * c + i] = T.at<float>(i / 4, i % 4);
        }
        for (int k = 0; k < K; ++k) {
            solver_n[k] = solvers[k]->Correspondences();
            solver_min[k] = solvers[k]->MinInliers();
            solver_its[k] = solvers[k]->MaxIterations();
            const std::vector<size_t> &ki = solvers[k]->KeyPointIndices();
            for (size_t i = 0; i < ki.size(); ++i) kp_index[(size_t)k * nslots + i] = (int32_t)ki[i];
            const std::vector<int32_t> &d = solvers[k]->Draws();
            if ((int)d.size() > 4 * draw_cap) throw std::runtime_error("more draws than the caller made room for");
            ndraws[k] = (int32_t)(d.size() / 4);
            for (size_t i = 0; i < d.size(); ++i) draws[(size_t)k * 4 * draw_cap + i] = d[i];
        }
        PnPsolver::SetHandle(NULL);
        return 0;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -1;
    }
}
