// tests/compat_recon: one extern "C" entry point around compat/Initializer_reconstruct.inl.  It fills an Initializer from flat
// arrays, calls ReconstructH or ReconstructF with R21, t21, vP3D and vbTriangulated pre-filled with marks (so that "left alone"
// can be told from "written") and returns what the call left.  Built twice by tests/test_compat_recon.py: with CR_SHARED_HANDLE
// the fragment runs on the handle the test passes in (ORBX_INITIALIZER_HANDLE), without it on the thread_local handle it creates
// for itself.  Every C++ exception is caught: -1 and cr_error().
#include <cstring>
#include <string>
#ifdef CR_SHARED_HANDLE
#include "orbx.h"
static orbx_handle *g_handle = NULL;
#define ORBX_INITIALIZER_HANDLE g_handle
#endif
#include "Initializer.h"

using namespace ORB_SLAM2;
static std::string g_error;
extern "C" const char *cr_error() { return g_error.c_str(); }

// shape [4]: R21 rows, R21 cols, vP3D.size(), vbTriangulated.size(); P3D [n1][3] and tri [n1] are written as far as the vectors
// reach.  Returns the function's return value (0 / 1), or -1.
extern "C" int cr_run(void *handle, int model, int n1, const float *keys1, int n2, const float *keys2, int n, const int32_t *matches,
                      const uint8_t *inliers, const float *M9, const float *K4, float sigma, float minParallax, int minTriangulated,
                      float *R9, float *t3, int32_t *shape, float *P3D, uint8_t *tri) {
    try {
#ifdef CR_SHARED_HANDLE
        g_handle = (orbx_handle *)handle;
#else
        (void)handle;
#endif
        Initializer I(sigma);
        I.mvKeys1.resize((size_t)n1); I.mvKeys2.resize((size_t)n2);
        for (int i = 0; i < n1; ++i) { I.mvKeys1[i].pt.x = keys1[2 * i]; I.mvKeys1[i].pt.y = keys1[2 * i + 1]; }
        for (int i = 0; i < n2; ++i) { I.mvKeys2[i].pt.x = keys2[2 * i]; I.mvKeys2[i].pt.y = keys2[2 * i + 1]; }
        std::vector<bool> inl((size_t)n);
        for (int i = 0; i < n; ++i) { I.mvMatches12.push_back(std::make_pair((int)matches[2 * i], (int)matches[2 * i + 1])); inl[i] = inliers[i] != 0; }
        cv::Mat M(3, 3, CV_32F), K = cv::Mat::zeros(3, 3, CV_32F), R21(1, 2, CV_32F), t21(1, 2, CV_32F);
        for (int i = 0; i < 9; ++i) M.at<float>(i / 3, i % 3) = M9[i];
        K.at<float>(0, 0) = K4[0]; K.at<float>(1, 1) = K4[1]; K.at<float>(0, 2) = K4[2]; K.at<float>(1, 2) = K4[3]; K.at<float>(2, 2) = 1.f;
        std::vector<cv::Point3f> vP3D(2, cv::Point3f(7.f, 7.f, 7.f));
        std::vector<bool> vbTriangulated(3, true);
        const bool ok = model == ORBX_INIT_H ? I.ReconstructH(inl, M, K, R21, t21, vP3D, vbTriangulated, minParallax, minTriangulated)
                                             : I.ReconstructF(inl, M, K, R21, t21, vP3D, vbTriangulated, minParallax, minTriangulated);
        shape[0] = R21.rows; shape[1] = R21.cols; shape[2] = (int32_t)vP3D.size(); shape[3] = (int32_t)vbTriangulated.size();
        if (ok) {
            if (R21.rows != 3 || R21.cols != 3 || t21.rows != 3 || t21.cols != 1) throw std::runtime_error("R21 or t21 has the wrong shape");
            for (int i = 0; i < 9; ++i) R9[i] = R21.at<float>(i / 3, i % 3);
            for (int i = 0; i < 3; ++i) t3[i] = t21.at<float>(i, 0);
        } else if (t21.rows != R21.rows || t21.cols != (R21.rows ? 2 : 0)) throw std::runtime_error("t21 was not treated as R21 was");
        for (size_t i = 0; i < vP3D.size() && i < (size_t)n1; ++i) { P3D[3 * i] = vP3D[i].x; P3D[3 * i + 1] = vP3D[i].y; P3D[3 * i + 2] = vP3D[i].z; }
        for (size_t i = 0; i < vbTriangulated.size() && i < (size_t)n1; ++i) tri[i] = vbTriangulated[i];
        return ok ? 1 : 0;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -1;
    }
}
