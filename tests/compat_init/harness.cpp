// tests/compat_init: one extern "C" entry point around compat/Initializer_ransac.inl.  It fills an Initializer from flat arrays
// (vMatches12 in the reference's form: one entry per keypoint of frame 1, -1 = unmatched, from which mvMatches12 is made as
// Initialize makes it, :116-131), runs the fragment and returns what it left.  Built twice by tests/test_compat_init.py: with
// CI_SHARED_HANDLE the fragment runs on the handle the test passes in (ORBX_INITIALIZER_HANDLE), without it on the
// thread_local handle it creates for itself.  Every C++ exception is caught: -1 and ci_error().
#include <cstring>
#include <string>
#ifdef CI_SHARED_HANDLE
#include "orbx.h"
static orbx_handle *g_handle = NULL;
#define ORBX_INITIALIZER_HANDLE g_handle
#endif
#include "Initializer.h"

using namespace ORB_SLAM2;
static std::string g_error;
extern "C" const char *ci_error() { return g_error.c_str(); }

// has [2]: whether H / F came back non-empty; inliers [2][n]; returns the number of matches, or -1
extern "C" int ci_run(void *handle, int n1, const float *keys1, int n2, const float *keys2, const int32_t *vMatches12, float sigma,
                      int iterations, const int32_t *sets, float *SH, float *SF, float *RH, float *H9, float *F9, int32_t *has,
                      uint8_t *inliersH, uint8_t *inliersF, int cap, int32_t *matches_out) {
    try {
#ifdef CI_SHARED_HANDLE
        g_handle = (orbx_handle *)handle;
#else
        (void)handle;
#endif
        Initializer I(sigma, iterations);
        I.mvKeys1.resize((size_t)n1); I.mvKeys2.resize((size_t)n2);
        for (int i = 0; i < n1; ++i) { I.mvKeys1[i].pt.x = keys1[2 * i]; I.mvKeys1[i].pt.y = keys1[2 * i + 1]; }
        for (int i = 0; i < n2; ++i) { I.mvKeys2[i].pt.x = keys2[2 * i]; I.mvKeys2[i].pt.y = keys2[2 * i + 1]; }
        for (int i = 0; i < n1; ++i)
            if (vMatches12[i] >= 0) I.mvMatches12.push_back(std::make_pair(i, (int)vMatches12[i]));
        const int N = (int)I.mvMatches12.size();
        if (N > cap) throw std::runtime_error("more matches than the output arrays hold");
        I.mvSets = std::vector<std::vector<size_t> >((size_t)iterations, std::vector<size_t>(8, 0));
        for (int it = 0; it < iterations; ++it)
            for (int j = 0; j < 8; ++j) I.mvSets[it][j] = (size_t)sets[8 * it + j];
        std::vector<bool> iH(3, true), iF(5, true);
        cv::Mat H, F;
        I.HF(iH, *SH, H, iF, *SF, F, *RH);
        if ((int)iH.size() != N || (int)iF.size() != N) throw std::runtime_error("a mask does not have one entry per match");
        for (int i = 0; i < N; ++i) {
            inliersH[i] = iH[i]; inliersF[i] = iF[i];
            matches_out[2 * i] = I.mvMatches12[i].first; matches_out[2 * i + 1] = I.mvMatches12[i].second;
        }
        has[0] = H.empty() ? 0 : 1; has[1] = F.empty() ? 0 : 1;
        for (int i = 0; i < 9; ++i) {
            H9[i] = H.empty() ? 0.f : H.at<float>(i / 3, i % 3);
            F9[i] = F.empty() ? 0.f : F.at<float>(i / 3, i % 3);
        }
        return N;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -1;
    }
}
