// tests/compat_rgbd: extern "C" entry point through which tests/test_rgbd.py runs compat/Frame_rgbd.inl.  The depth image is a
// CV_32F view of `stride` floats per row (a column range of a wider matrix when stride > width), as GrabImageRGBD may leave it.
// Returns 0, or -1 after any C++ exception, whose text rgbd_error() then returns.
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "Frame.h"
namespace ORB_SLAM2 {
#include "Frame_rgbd.inl"
}

using namespace ORB_SLAM2;

namespace {
std::string g_error;
std::unique_ptr<ORBextractor> g_ex;
}  // namespace

extern "C" {
const char *rgbd_error() { return g_error.c_str(); }

int rgbd_compute(const void *kps, const void *kps_un, int n, float *depth, int width, int height, int stride_floats, float mbf,
                 float *u_right, float *depth_out) {
    try {
        if (!g_ex) g_ex.reset(new ORBextractor(1000, 1.2f, 8, 20, 7));
        Frame F;
        F.mpORBextractorLeft = g_ex.get();
        F.mbf = mbf;
        F.N = n;
        const cv::KeyPoint *k = static_cast<const cv::KeyPoint *>(kps), *ku = static_cast<const cv::KeyPoint *>(kps_un);
        F.mvKeys.assign(k, k + n);
        F.mvKeysUn.assign(ku, ku + n);
        const cv::Mat wide(height, stride_floats, CV_32F, depth);
        F.ComputeStereoFromRGBD(wide.colRange(0, width));
        if (F.mvuRight.size() != (size_t)n || F.mvDepth.size() != (size_t)n) throw std::runtime_error("output sizes differ from N");
        if (n) {
            std::memcpy(u_right, F.mvuRight.data(), (size_t)n * sizeof(float));
            std::memcpy(depth_out, F.mvDepth.data(), (size_t)n * sizeof(float));
        }
        return 0;
    } catch (const std::exception &e) {
        g_error = e.what();
    } catch (...) {
        g_error = "unknown exception";
    }
    return -1;
}
}
