// compat/Frame_rgbd.inl -- replacement BODY for Frame::ComputeStereoFromRGBD (reference src/Frame.cc:1179-1226), the depth step
// of the RGB-D Frame constructor (:237-321).
//
// How to apply (maintainer, inside the ORB-SLAM2 tree; needs OpenCV -- this repository's tests run the body against working
// stand-ins, tests/compat_rgbd/, and the maintainer's build remains the final check):
//   in src/Frame.cc, delete the body of Frame::ComputeStereoFromRGBD and put   #include "Frame_rgbd.inl"   in its place, inside
//   namespace ORB_SLAM2.  Nothing else changes: the constructor still runs ExtractORB and UndistortKeyPoints before it.
//
// Tracking::GrabImageRGBD (src/Tracking.cc:327-332) has already turned imDepth into CV_32F with mDepthMapFactor applied, so the
// body passes float depth with scale 1.  orbx_rgbd_depth then reads the pixel the reference's imDepth.at<float>(v, u) reads at
// the distorted keypoint, row wrap included, and gives no depth where that read lies past the image (F7, DESIGN.md section 2:
// the reference's read is undefined behaviour there).  mvuRight / mvDepth come back as the reference leaves them (-1 where
// there is no depth).
void Frame::ComputeStereoFromRGBD(const cv::Mat &imDepth)
{
    mvuRight = std::vector<float>(N, -1);
    mvDepth = std::vector<float>(N, -1);
    if (N == 0) return;
    if (imDepth.type() != CV_32F) throw std::runtime_error("ComputeStereoFromRGBD: imDepth must be CV_32F (see GrabImageRGBD)");
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint must be the 28-byte POD");
    const orbx_status st = orbx_rgbd_depth(
        mpORBextractorLeft->handle(), reinterpret_cast<const orbx_keypoint *>(mvKeys.data()),
        reinterpret_cast<const orbx_keypoint *>(mvKeysUn.data()), N, imDepth.ptr<float>(), ORBX_DEPTH_F32, imDepth.cols,
        imDepth.rows, (int)imDepth.step, 1.0f, mbf, mvuRight.data(), mvDepth.data());
    if (st != ORBX_OK) throw std::runtime_error(orbx_last_error());
}
