// compat/MapPoint_batch.inl -- BODY of one static member the maintainer adds to MapPoint (reference include/MapPoint.h):
//
//     static void RefreshBatch(const std::vector<MapPoint *> &vpMPs, bool bDescriptors, bool bNormalAndDepth);
//
// How to apply (maintainer, inside the ORB-SLAM2 tree; needs OpenCV -- this repository's tests run the body against working
// stand-ins, tests/compat_mappoint/, and the maintainer's build remains the final check): declare the member as above, put
//   #include "MapPoint_batch.inl"   into src/MapPoint.cc inside namespace ORB_SLAM2 (with <set>, <cstring>, <stdexcept> and
// "orbx.h" included above it), and replace the loops that end with
//     pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth();
// on every point they touched (INTEGRATION.md lists them) by collecting the points and calling RefreshBatch once behind the
// loop.  Inside these loops the points are independent, so the batch equals the loop.  A single call outside a loop stays on the
// host: one round trip to the device costs more than one point.
//
// For each non-NULL point, once (a point that appears twice is computed once), the body snapshots under the reference's locks
// what the two functions snapshot (src/MapPoint.cc:424-463 and :570-590): the observations, for the descriptor the rows of the
// keyframes that are not bad in the map's iteration order, for the normal every observing keyframe's camera centre, the
// reference keyframe's centre and the octave of the point's keypoint in it.  A point the reference returns early for (bad, no
// observations, for the descriptor also: every keyframe bad) gets no rows and is left as it is.  Then one
// orbx_distinctive_descriptors_batch and / or one orbx_update_normal_and_depth_batch call, and mDescriptor, mNormalVector,
// mfMinDistance, mfMaxDistance are written under the locks the reference writes them under.  The handle belongs to the calling
// thread and carries the keyframes' scale factor and level count.

void MapPoint::RefreshBatch(const std::vector<MapPoint *> &vpMPs, bool bDescriptors, bool bNormalAndDepth)
{
    std::vector<MapPoint *> pts;
    {
        std::set<MapPoint *> seen;
        for (size_t i = 0; i < vpMPs.size(); ++i)
            if (vpMPs[i] && seen.insert(vpMPs[i]).second) pts.push_back(vpMPs[i]);
    }
    const int P = (int)pts.size();
    if (P == 0 || (!bDescriptors && !bNormalAndDepth)) return;

    std::vector<std::map<KeyFrame *, size_t> > obs((size_t)P);
    std::vector<KeyFrame *> ref((size_t)P, static_cast<KeyFrame *>(NULL));
    std::vector<float> pos((size_t)P * 3, 0.f);
    KeyFrame *anyKF = NULL;
    for (int k = 0; k < P; ++k) {
        MapPoint *p = pts[k];
        std::unique_lock<std::mutex> lock1(p->mMutexFeatures);
        std::unique_lock<std::mutex> lock2(p->mMutexPos);
        if (p->mbBad) continue;
        obs[k] = p->mObservations;
        ref[k] = p->mpRefKF;
        for (int c = 0; c < 3; ++c) pos[3 * (size_t)k + c] = p->mWorldPos.at<float>(c);
        if (!obs[k].empty()) anyKF = obs[k].begin()->first;
    }
    if (!anyKF) return;                                              // every point is bad or unobserved

    struct Holder { orbx_handle *h = NULL; float factor = 0.f; int levels = 0; ~Holder() { orbx_destroy(h); } };
    thread_local Holder t;
    if (!t.h || t.factor != anyKF->mfScaleFactor || t.levels != anyKF->mnScaleLevels) {
        orbx_destroy(t.h);
        t.h = NULL;
        orbx_params prm;
        orbx_default_params(&prm);
        prm.scale_factor = anyKF->mfScaleFactor;
        prm.nlevels = anyKF->mnScaleLevels;
        if (orbx_create(&prm, &t.h) != ORBX_OK) throw std::runtime_error(orbx_last_error());
        t.factor = anyKF->mfScaleFactor; t.levels = anyKF->mnScaleLevels;
    }

    std::vector<int32_t> begin((size_t)P + 1, 0);
    if (bDescriptors) {
        std::vector<uint8_t> rows;
        for (int k = 0; k < P; ++k) {
            for (std::map<KeyFrame *, size_t>::iterator mit = obs[k].begin(); mit != obs[k].end(); ++mit) {
                KeyFrame *pKF = mit->first;
                if (pKF->isBad()) continue;
                const uint8_t *d = pKF->mDescriptors.ptr<uint8_t>((int)mit->second);
                rows.insert(rows.end(), d, d + 32);
            }
            begin[(size_t)k + 1] = (int32_t)(rows.size() / 32);
        }
        std::vector<int32_t> best((size_t)P, -1);
        std::vector<uint8_t> out((size_t)P * 32, 0);
        if (orbx_distinctive_descriptors_batch(t.h, P, begin.data(), rows.empty() ? NULL : rows.data(), best.data(), NULL,
                                               out.data()) != ORBX_OK)
            throw std::runtime_error(orbx_last_error());
        for (int k = 0; k < P; ++k) {
            if (best[k] < 0) continue;
            cv::Mat d(1, 32, CV_8U);
            std::memcpy(d.ptr<uint8_t>(), &out[(size_t)k * 32], 32);
            std::unique_lock<std::mutex> lock(pts[k]->mMutexFeatures);
            pts[k]->mDescriptor = d;
        }
    }
    if (bNormalAndDepth) {
        std::vector<float> centers, refc((size_t)P * 3, 0.f);
        std::vector<int32_t> level((size_t)P, 0);
        for (int k = 0; k < P; ++k) {
            for (std::map<KeyFrame *, size_t>::iterator mit = obs[k].begin(); mit != obs[k].end(); ++mit) {
                const cv::Mat Owi = mit->first->GetCameraCenter();   // bad keyframes included, as :597-612
                for (int c = 0; c < 3; ++c) centers.push_back(Owi.at<float>(c));
            }
            begin[(size_t)k + 1] = (int32_t)(centers.size() / 3);
            if (obs[k].empty()) continue;
            const cv::Mat Or = ref[k]->GetCameraCenter();
            for (int c = 0; c < 3; ++c) refc[3 * (size_t)k + c] = Or.at<float>(c);
            const std::map<KeyFrame *, size_t>::iterator mref = obs[k].find(ref[k]);
            level[k] = ref[k]->mvKeysUn[mref == obs[k].end() ? 0 : mref->second].octave;   // observations[pRefKF], :620
        }
        std::vector<float> normal((size_t)P * 3, 0.f), dmin((size_t)P, 0.f), dmax((size_t)P, 0.f);
        if (orbx_update_normal_and_depth_batch(t.h, P, begin.data(), pos.data(), centers.empty() ? NULL : centers.data(), refc.data(),
                                               level.data(), normal.data(), dmin.data(), dmax.data()) != ORBX_OK)
            throw std::runtime_error(orbx_last_error());
        for (int k = 0; k < P; ++k) {
            if (obs[k].empty()) continue;
            cv::Mat n(3, 1, CV_32F);
            for (int c = 0; c < 3; ++c) n.at<float>(c) = normal[3 * (size_t)k + c];
            std::unique_lock<std::mutex> lock3(pts[k]->mMutexPos);
            pts[k]->mfMaxDistance = dmax[k];
            pts[k]->mfMinDistance = dmin[k];
            pts[k]->mNormalVector = n;
        }
    }
}
