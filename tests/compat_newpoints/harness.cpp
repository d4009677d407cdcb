// tests/compat_newpoints: one extern "C" entry point around compat/LocalMapping_newpoints.inl.  It fills two keyframes from flat
// arrays, runs one pass of the neighbour loop and returns what the fragment left: per created MapPoint, in creation order, the
// position and the two observation indices, after checking on the spot that everything :655-677 does was done to it.  Built
// twice by tests/test_compat_newpoints.py: with CN_SHARED_HANDLE the fragment runs on the handle the test passes in
// (ORBX_LOCALMAPPING_HANDLE), without it on the thread_local handles it creates for itself.  Every C++ exception is caught: -1 and
// cn_error().
#include <cstring>
#include <string>
#ifdef CN_SHARED_HANDLE
#include "orbx.h"
static orbx_handle *g_handle = NULL;
#define ORBX_LOCALMAPPING_HANDLE g_handle
#endif
#include "LocalMapping.h"

using namespace ORB_SLAM2;
static std::string g_error;
extern "C" const char *cn_error() { return g_error.c_str(); }

// pose [15]: Rcw, tcw, Ow; cam [8]: fx fy cx cy invfx invfy mb mbf; un [n][3]: x y octave; keys [n][2]
static void fill(KeyFrame &K, const float *pose, const float *cam, int nlevels, const float *sf, const float *s2, int n,
                 const float *un, const float *keys, const float *ur, const float *depth) {
    K.Rcw = cv::Mat(3, 3, CV_32F); K.tcw = cv::Mat(3, 1, CV_32F); K.Ow = cv::Mat(3, 1, CV_32F);
    for (int i = 0; i < 9; ++i) K.Rcw.at<float>(i / 3, i % 3) = pose[i];
    for (int i = 0; i < 3; ++i) { K.tcw.at<float>(i) = pose[9 + i]; K.Ow.at<float>(i) = pose[12 + i]; }
    K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.invfx = cam[4]; K.invfy = cam[5]; K.mb = cam[6]; K.mbf = cam[7];
    K.mvScaleFactors.assign(sf, sf + nlevels); K.mvLevelSigma2.assign(s2, s2 + nlevels);
    K.mvKeysUn.resize((size_t)n); K.mvKeys.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        K.mvKeysUn[i].pt.x = un[3 * i]; K.mvKeysUn[i].pt.y = un[3 * i + 1]; K.mvKeysUn[i].octave = (int)un[3 * i + 2];
        K.mvKeys[i].pt.x = keys[2 * i]; K.mvKeys[i].pt.y = keys[2 * i + 1]; K.mvKeys[i].octave = (int)un[3 * i + 2];
    }
    K.mvuRight.assign(ur, ur + n); K.mvDepth.assign(depth, depth + n);
    K.mvpMapPoints.assign((size_t)n, static_cast<MapPoint *>(NULL));
}

// Returns the number of MapPoints created (= nnew), or -1.  points [nmatches][3], obs [nmatches][2] are filled that far.
extern "C" int cn_run(void *handle, float scale_factor, const float *pose1, const float *cam1, int nlevels1, const float *sf1,
                      const float *s21, int n1, const float *un1, const float *keys1, const float *ur1, const float *depth1,
                      const float *pose2, const float *cam2, int nlevels2, const float *sf2, const float *s22, int n2, const float *un2,
                      const float *keys2, const float *ur2, const float *depth2, int nmatches, const int32_t *matches, float *points,
                      int32_t *obs) {
    try {
#ifdef CN_SHARED_HANDLE
        g_handle = (orbx_handle *)handle;
#else
        (void)handle;
#endif
        KeyFrame K1, K2;
        fill(K1, pose1, cam1, nlevels1, sf1, s21, n1, un1, keys1, ur1, depth1);
        fill(K2, pose2, cam2, nlevels2, sf2, s22, n2, un2, keys2, ur2, depth2);
        K1.mfScaleFactor = scale_factor; K2.mfScaleFactor = scale_factor;
        Map map;
        LocalMapping LM(&map, &K1);
        std::vector<std::pair<size_t, size_t> > v;
        for (int i = 0; i < nmatches; ++i) v.push_back(std::make_pair((size_t)matches[2 * i], (size_t)matches[2 * i + 1]));
        const int nnew = LM.CreateNewMapPointsFor(&K2, v);
        if ((int)map.mvpMapPoints.size() != nnew || (int)LM.mlpRecentAddedMapPoints.size() != nnew) throw std::runtime_error("nnew, the map and the recent list disagree");
        std::list<MapPoint *>::const_iterator it = LM.mlpRecentAddedMapPoints.begin();
        for (int j = 0; j < nnew; ++j, ++it) {
            MapPoint *p = map.mvpMapPoints[(size_t)j];
            if (*it != p) throw std::runtime_error("the recent list is not in creation order");
            if (p->mpRefKF != &K1 || p->mpMap != &map || p->mnDistinctive != 1 || p->mnNormal != 1) throw std::runtime_error("a MapPoint was not set up as :655-669 does");
            if (p->mObservations.size() != 2 || p->mObservations[0].first != &K1 || p->mObservations[1].first != &K2) throw std::runtime_error("observations");
            const size_t i1 = p->mObservations[0].second, i2 = p->mObservations[1].second;
            if (K1.mvpMapPoints.at(i1) != p || K2.mvpMapPoints.at(i2) != p) throw std::runtime_error("AddMapPoint was not called on both keyframes");
            if (p->mWorldPos.rows != 3 || p->mWorldPos.cols != 1) throw std::runtime_error("x3D has the wrong shape");
            for (int c = 0; c < 3; ++c) points[3 * j + c] = p->mWorldPos.at<float>(c);
            obs[2 * j] = (int32_t)i1; obs[2 * j + 1] = (int32_t)i2;
        }
        for (size_t j = 0; j < map.mvpMapPoints.size(); ++j) delete map.mvpMapPoints[j];
        return nnew;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -1;
    }
}
