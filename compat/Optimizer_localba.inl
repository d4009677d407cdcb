// compat/Optimizer_localba.inl -- replacement for the BODY of Optimizer::LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag,
// Map *pMap) from "Setup optimizer" to the end (reference src/Optimizer.cc:710-1030).  The statements before it (:636-708), which
// collect lLocalKeyFrames, lLocalMapPoints and lFixedCameras, stay the reference's.
//
// How to apply (maintainer, inside the ORB-SLAM2 tree; needs OpenCV): in src/Optimizer.cc, delete :710-1029 and put
//   #include "Optimizer_localba.inl"   in their place, inside the function, with <map>, <vector>, <stdexcept> and "orbx.h"
// included at the top of the file, and MapPoint::RefreshBatch declared and defined as compat/MapPoint_batch.inl describes.  No
// g2o is left in that function.  This repository's tests run the fragment against working stand-ins (tests/compat_localba/)
// on a host-only handle; the maintainer's build remains the final check.
//
// The fragment flattens the three lists under the mutexes the reference takes (GetPose, GetWorldPos, GetObservations each lock
// inside), leaving out bad keyframes (:813); reads the stop flag where the reference does -- set before the optimisation: return
// (:886-888); it cannot be sampled between the rounds of one call, so bDoMore is true whenever the call is made --; makes ONE
// orbx_local_bundle_adjustment_batch call; applies vToErase under mMutexMapUpdate, skipping points that have gone bad since the
// snapshot (the reference skips them inside its classification loops); calls SetPose / SetWorldPos; and refreshes the points
// with MapPoint::RefreshBatch(points, false, true) in place of the per-point UpdateNormalAndDepth.
// One local map is one call on the library's HOST path (a host-only handle created on first use): measured on an MI355X, a lone
// problem takes 8.0 / 64 ms on the device against 3.9 / 24 ms on the host path (8 + 8 keyframes, 600 points / 25 + 20
// keyframes, 2000 points); from 4 problems per call on the device wins (profiles/localba_batch.md).  A multi-stream mapper
// calls orbx_local_bundle_adjustment_batch on a device handle with all its streams' problems instead.
// More than 128 local keyframes: the call returns ORBX_UNSUPPORTED and the fragment throws.
// Parity: the result equals tests/localba_model.py bit for bit; parity with the g2o + Eigen body is not pinned (DESIGN.md section
// 2, F19).
{
    struct HostHandle {
        orbx_handle *h = NULL;
        HostHandle() {
            orbx_params p;
            orbx_default_params(&p);
            p.device = -2;                                // host-only: the library's host path
            if (orbx_create(&p, &h) != ORBX_OK) throw std::runtime_error(orbx_last_error());
        }
        ~HostHandle() { orbx_destroy(h); }
    };
    static HostHandle host;

    std::vector<KeyFrame *> vpKFs;                        // the local keyframes in list order, then the fixed ones
    std::map<KeyFrame *, int32_t> kfIndex;
    std::vector<float> vTcw;
    std::vector<uint8_t> vLocalFixed;
    for (list<KeyFrame *>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        kfIndex[*lit] = (int32_t)vpKFs.size();
        vpKFs.push_back(*lit);
        vLocalFixed.push_back((*lit)->mnId == 0 ? 1 : 0);
    }
    const int nLocal = (int)vpKFs.size();
    for (list<KeyFrame *>::iterator lit = lFixedCameras.begin(), lend = lFixedCameras.end(); lit != lend; lit++) {
        kfIndex[*lit] = (int32_t)vpKFs.size();
        vpKFs.push_back(*lit);
    }
    for (size_t k = 0; k < vpKFs.size(); k++) {
        const cv::Mat Tcw = vpKFs[k]->GetPose();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) vTcw.push_back(Tcw.at<float>(r, c));
    }

    std::vector<MapPoint *> vpMPs;
    std::vector<float> vWorld, vObs, vInvSigma2;
    std::vector<int32_t> vObsBegin(1, 0), vObsKF;
    std::vector<KeyFrame *> vpEdgeKF;
    std::vector<MapPoint *> vpEdgeMP;
    for (list<MapPoint *>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        MapPoint *pMP = *lit;
        vpMPs.push_back(pMP);
        const cv::Mat Pos = pMP->GetWorldPos();
        for (int c = 0; c < 3; c++) vWorld.push_back(Pos.at<float>(c));
        const map<KeyFrame *, size_t> observations = pMP->GetObservations();
        for (map<KeyFrame *, size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
            KeyFrame *pKFi = mit->first;
            if (pKFi->isBad()) continue;
            const std::map<KeyFrame *, int32_t>::const_iterator at = kfIndex.find(pKFi);
            if (at == kfIndex.end()) continue;            // (cannot happen: :685-706 put every observer into one of the lists)
            const cv::KeyPoint &kpUn = pKFi->mvKeysUn[mit->second];
            vObsKF.push_back(at->second);
            vObs.push_back(kpUn.pt.x); vObs.push_back(kpUn.pt.y); vObs.push_back(pKFi->mvuRight[mit->second]);
            vInvSigma2.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
            vpEdgeKF.push_back(pKFi);
            vpEdgeMP.push_back(pMP);
        }
        vObsBegin.push_back((int32_t)vObsKF.size());
    }

    if (pbStopFlag)
        if (*pbStopFlag)
            return;

    std::vector<float> vTcwOut((size_t)nLocal * 16, 0.f), vWorldOut(vWorld.size(), 0.f);
    std::vector<uint8_t> vErase(vObsKF.size(), 0);
    orbx_localba_problem P;
    P.nlocal = nLocal; P.nfixed = (int32_t)vpKFs.size() - nLocal; P.npoints = (int32_t)vpMPs.size();
    P.second_round = 1;
    P.Tcw = vTcw.data(); P.local_fixed = vLocalFixed.data();
    P.camera[0] = pKF->fx; P.camera[1] = pKF->fy; P.camera[2] = pKF->cx; P.camera[3] = pKF->cy;
    P.bf = pKF->mbf;
    P.world = vWorld.data();
    P.obs_begin = vObsBegin.data(); P.obs_kf = vObsKF.data(); P.obs = vObs.data(); P.inv_sigma2 = vInvSigma2.data();
    P.Tcw_out = vTcwOut.data(); P.world_out = vWorldOut.data(); P.erase = vErase.data();
    orbx_localba_result res;
    if (orbx_local_bundle_adjustment_batch(host.h, 1, &P, &res) != ORBX_OK) throw std::runtime_error(orbx_last_error());

    // Get Map Mutex
    unique_lock<mutex> lock(pMap->mMutexMapUpdate);

    for (size_t i = 0; i < vErase.size(); i++) {
        if (!vErase[i] || vpEdgeMP[i]->isBad()) continue;
        vpEdgeKF[i]->EraseMapPointMatch(vpEdgeMP[i]);
        vpEdgeMP[i]->EraseObservation(vpEdgeKF[i]);
    }

    // Recover optimized data
    for (int k = 0; k < nLocal; k++) {
        cv::Mat Tcw(4, 4, CV_32F);
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) Tcw.at<float>(r, c) = vTcwOut[16 * (size_t)k + 4 * r + c];
        vpKFs[k]->SetPose(Tcw);
    }
    for (size_t p = 0; p < vpMPs.size(); p++) {
        cv::Mat Pos(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) Pos.at<float>(c) = vWorldOut[3 * p + c];
        vpMPs[p]->SetWorldPos(Pos);
    }
    MapPoint::RefreshBatch(vpMPs, false, true);
}
