// tests/compat_sim3: one extern "C" entry point around compat/Sim3Solver.h.  It builds the current keyframe (nslots MapPoint
// slots) and K candidate keyframes from flat arrays, one Sim3Solver per candidate, optionally Sim3Solver::Prepare, then plays
// ncalls iterate(call_n) calls on solver call_k and returns what each gave.  Every C++ exception is caught: -1 and cs_error().
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "Sim3Solver.h"

using namespace ORB_SLAM2;
static std::string g_error;
extern "C" const char *cs_error() { return g_error.c_str(); }

static cv::Mat pose(const float *T) {
    cv::Mat m(4, 4, CV_32F);
    for (int i = 0; i < 16; ++i) m.at<float>(i / 4, i % 4) = T[i];
    return m;
}
static cv::Mat vec3(const float *p) {
    cv::Mat m(3, 1, CV_32F);
    for (int i = 0; i < 3; ++i) m.at<float>(i) = p[i];
    return m;
}

// state1 / state2 [K][nslots]: 0 = a sound point, 1 = NULL, 2 = bad, 3 = not observed by its keyframe.  state2 == 1: no match.
extern "C" int cs_run(void *handle, int K, int nslots, const uint8_t *state1, const uint8_t *state2, const float *pos1,
                      const float *pos2, const int32_t *oct1, const int32_t *oct2, const float *T1, const float *T2,
                      const float *K1, const float *K2, int fix_scale, double probability, int min_inliers, int max_iterations,
                      uint64_t seed, int prepare, int ncalls, const int32_t *call_k, const int32_t *call_n,
                      int32_t *ret, int32_t *no_more, int32_t *ninliers, float *T12, uint8_t *inliers, int32_t *best_ok, float *best,
                      int32_t *solver_n, int32_t *solver_its, int32_t *draws) {
    try {
        Sim3Solver::SetHandle((orbx_handle *)handle);
        DUtils::Random::State() = seed;
        std::vector<std::unique_ptr<MapPoint>> points;
        std::vector<std::unique_ptr<KeyFrame>> kfs;
        std::vector<std::unique_ptr<Sim3Solver>> solvers;
        std::vector<Sim3Solver *> list;
        for (int k = 0; k < K; ++k) {
            // LoopClosing builds one solver per candidate against the same current keyframe; here every candidate gets a current
            // keyframe of its own so that the slot states can differ per candidate
            kfs.emplace_back(new KeyFrame(pose(T1), K1, 8, 1.2f));
            KeyFrame *kf1 = kfs.back().get();
            kfs.emplace_back(new KeyFrame(pose(T2 + 16 * k), K2 + 4 * k, 8, 1.2f));
            KeyFrame *kf2 = kfs.back().get();
            std::vector<MapPoint *> matched((size_t)nslots, static_cast<MapPoint *>(NULL));
            kf1->mvpMapPoints.assign((size_t)nslots, static_cast<MapPoint *>(NULL));
            kf1->mvKeysUn.resize((size_t)nslots); kf2->mvKeysUn.resize((size_t)nslots);
            for (int i = 0; i < nslots; ++i) {
                const size_t e = (size_t)k * nslots + i;
                kf1->mvKeysUn[i].octave = oct1[e]; kf2->mvKeysUn[i].octave = oct2[e];
                if (state1[e] != 1) {
                    points.emplace_back(new MapPoint(vec3(pos1 + 3 * e), state1[e] == 2));
                    if (state1[e] != 3) points.back()->AddObservation(kf1, i);
                    kf1->mvpMapPoints[i] = points.back().get();
                }
                if (state2[e] != 1) {
                    points.emplace_back(new MapPoint(vec3(pos2 + 3 * e), state2[e] == 2));
                    if (state2[e] != 3) points.back()->AddObservation(kf2, i);
                    matched[i] = points.back().get();
                }
            }
            solvers.emplace_back(new Sim3Solver(kf1, kf2, matched, fix_scale != 0));
            solvers.back()->SetRansacParameters(probability, min_inliers, max_iterations);
            list.push_back(solvers.back().get());
        }
        if (prepare) Sim3Solver::Prepare(list);
        for (int c = 0; c < ncalls; ++c) {
            Sim3Solver &S = *solvers[call_k[c]];
            bool bNoMore = false;
            std::vector<bool> vbInliers;
            int nInliers = -1;
            const cv::Mat Scm = S.iterate(call_n[c], bNoMore, vbInliers, nInliers);
            ret[c] = Scm.empty() ? 0 : 1;
            no_more[c] = bNoMore ? 1 : 0;
            ninliers[c] = nInliers;
            if ((int)vbInliers.size() != nslots) throw std::runtime_error("vbInliers does not have mN1 entries");
            for (int i = 0; i < nslots; ++i) inliers[(size_t)c * nslots + i] = vbInliers[i] ? 1 : 0;
            if (!Scm.empty())
                for (int i = 0; i < 16; ++i) T12[16 * c + i] = Scm.at<float>(i / 4, i % 4);
            const cv::Mat R = S.GetEstimatedRotation(), t = S.GetEstimatedTranslation();
            best_ok[c] = R.empty() ? 0 : 1;
            if (!R.empty()) {
                for (int i = 0; i < 9; ++i) best[13 * c + i] = R.at<float>(i / 3, i % 3);
                for (int i = 0; i < 3; ++i) best[13 * c + 9 + i] = t.at<float>(i);
                best[13 * c + 12] = S.GetEstimatedScale();
            }
        }
        for (int k = 0; k < K; ++k) {
            solver_n[k] = solvers[k]->Correspondences();
            solver_its[k] = solvers[k]->MaxIterations();
            const std::vector<int32_t> &d = solvers[k]->Draws();
            if ((int)d.size() > 3 * max_iterations) throw std::runtime_error("more draws than iterations");
            for (size_t i = 0; i < (size_t)3 * max_iterations; ++i) draws[(size_t)k * 3 * max_iterations + i] = i < d.size() ? d[i] : -1;
        }
        Sim3Solver::SetHandle(NULL);
        return 0;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -1;
    }
}
