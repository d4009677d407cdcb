// compat/Optimizer_essentialgraph.inl -- replacement for the BODY of Optimizer::OptimizeEssentialGraph(Map *pMap, KeyFrame
// *pLoopKF, KeyFrame *pCurKF, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3, const LoopClosing::KeyFrameAndPose
// &CorrectedSim3, const map<KeyFrame *, set<KeyFrame *>> &LoopConnections, const bool &bFixScale) from "Set KeyFrame vertices"
// to the end (reference src/Optimizer.cc:1090-1357).  Of the statements before it the fragment reads vpKFs, vpMPs, nMaxKFid and
// minFeat (:1070-1084); the g2o set-up (:1057-1067) and vScw, vCorrectedSwc, vpVertices (:1077-1081) can go.
//
// How to apply (maintainer, inside the ORB-SLAM2 tree; needs OpenCV): in src/Optimizer.cc, delete :1090-1357 and put
//   #include "Optimizer_essentialgraph.inl"   in their place, inside the function, with <map>, <set>, <vector>, <stdexcept> and
// "orbx.h" included at the top of the file, and MapPoint::RefreshBatch declared and defined as compat/MapPoint_batch.inl
// describes.  This repository's tests run the fragment against working stand-ins (tests/compat_essgraph/) on a host-only
// handle; the maintainer's build remains the final check.
//
// The reference's own loops build the arrays: step 2 gives every keyframe that is not bad a vertex (CorrectedSim3 where it has
// one, else orbx_essgraph_sim3_from_tcw of its pose, scale 1), steps 3 and 4 push (i, j, kind) where the reference adds an
// EdgeSim3 -- the library computes the measurements -- and step 7's choice of the reference keyframe gives every point its
// vertex.  The reference dereferences optimizer.vertex(id) of a bad keyframe at :1166 / :1215 / :1244 / :1283 and :1308; the
// fragment leaves out an edge whose other end is bad, gives a bad keyframe no SetPose, and leaves a point whose reference
// keyframe is bad where it is (the reference maps it through two default-constructed Sim3: the identity, up to rounding).
// ONE orbx_optimize_essential_graph_batch call on the library's HOST path (a host-only handle created on first use): measured
// on an MI355X a lone problem takes 17.5 / 57 / 134 ms on the device against 10.0 / 49 / 150 ms on the host path (chains of 100 /
// 400 / 1500 keyframes with covisibility edges): it loses up to a few hundred keyframes and gains a tenth at 1500; from 4
// problems per call on the device wins at every size (profiles/essgraph_batch.md).  A caller with several loop closures in
// flight calls orbx_optimize_essential_graph_batch on a device handle with all of them instead.
// The host path has no cap on the blocks of L.
// Parity: the result equals tests/essgraph_model.py bit for bit; parity with the g2o + Eigen body is not pinned (DESIGN.md
// section 2, F20).
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

    // Step 2: a vertex for every keyframe that is not bad
    std::vector<KeyFrame *> vpVertexKF;
    std::vector<int32_t> vnVertex(nMaxKFid + 1, -1);      // mnId -> vertex, -1: a bad keyframe
    std::vector<double> vScw8, vNonCorrected8;
    std::vector<uint8_t> vFixed, vHasNonCorrected;
    struct Push {
        static void sim3(std::vector<double> &v, const g2o::Sim3 &S) {
            v.push_back(S.rotation().x()); v.push_back(S.rotation().y()); v.push_back(S.rotation().z()); v.push_back(S.rotation().w());
            for (int k = 0; k < 3; k++) v.push_back(S.translation()[k]);
            v.push_back(S.scale());
        }
    };
    for (size_t k = 0; k < vpKFs.size(); k++) {
        KeyFrame *kf = vpKFs[k];
        if (kf->isBad()) continue;
        vnVertex[kf->mnId] = (int32_t)vpVertexKF.size();
        vpVertexKF.push_back(kf);
        vFixed.push_back(kf == pLoopKF ? 1 : 0);
        const LoopClosing::KeyFrameAndPose::const_iterator corrected = CorrectedSim3.find(kf);
        if (corrected != CorrectedSim3.end()) {
            Push::sim3(vScw8, corrected->second);
        } else {                                          // the tracked pose with scale 1
            const cv::Mat Tcw = kf->GetPose();
            float T[16];
            double S[8];
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) T[4 * r + c] = Tcw.at<float>(r, c);
            orbx_essgraph_sim3_from_tcw(T, S);
            vScw8.insert(vScw8.end(), S, S + 8);
        }
        const LoopClosing::KeyFrameAndPose::const_iterator tracked = NonCorrectedSim3.find(kf);
        vHasNonCorrected.push_back(tracked != NonCorrectedSim3.end() ? 1 : 0);
        if (tracked != NonCorrectedSim3.end()) Push::sim3(vNonCorrected8, tracked->second);
        else vNonCorrected8.insert(vNonCorrected8.end(), 8, 0.0);
    }

    // Steps 3 and 4 push (i, j, kind) where the reference adds an EdgeSim3; an edge with a bad end is left out
    typedef std::pair<long unsigned int, long unsigned int> IdPair;
    std::vector<int32_t> vEdges;
    std::set<IdPair> sGuarded;                            // sInsertedEdges: consulted by the covisibility edges only
    struct Graph {
        std::vector<int32_t> &edges;
        const std::vector<int32_t> &vertex;
        int32_t of(KeyFrame *kf) const { return kf ? vertex[kf->mnId] : -1; }
        bool add(KeyFrame *from, KeyFrame *to, int32_t kind) {
            const int32_t a = of(from), b = of(to);
            if (a < 0 || b < 0) return false;
            edges.push_back(a); edges.push_back(b); edges.push_back(kind);
            return true;
        }
        static IdPair ids(KeyFrame *a, KeyFrame *b) { return a->mnId < b->mnId ? IdPair(a->mnId, b->mnId) : IdPair(b->mnId, a->mnId); }
    } graph = {vEdges, vnVertex};

    // Step 3 (:1139-1177): the loop connections -- the closing pair whatever its weight, the others from minFeat on
    for (std::map<KeyFrame *, std::set<KeyFrame *> >::const_iterator conn = LoopConnections.begin(); conn != LoopConnections.end(); ++conn) {
        KeyFrame *from = conn->first;
        for (std::set<KeyFrame *>::const_iterator to = conn->second.begin(); to != conn->second.end(); ++to) {
            const bool closing = from->mnId == pCurKF->mnId && (*to)->mnId == pLoopKF->mnId;
            if (!closing && from->GetWeight(*to) < minFeat) continue;
            if (graph.add(from, *to, 1)) sGuarded.insert(Graph::ids(from, *to));
        }
    }

    // Step 4 (:1181-1291): spanning tree, earlier loop edges, strong covisibility
    for (size_t k = 0; k < vpKFs.size(); k++) {
        KeyFrame *kf = vpKFs[k];
        if (kf->isBad()) continue;
        KeyFrame *parent = kf->GetParent();
        graph.add(kf, parent, 0);
        const std::set<KeyFrame *> loops = kf->GetLoopEdges();
        for (std::set<KeyFrame *>::const_iterator l = loops.begin(); l != loops.end(); ++l)
            if ((*l)->mnId < kf->mnId) graph.add(kf, *l, 0);
        const std::vector<KeyFrame *> strong = kf->GetCovisiblesByWeight(minFeat);
        for (size_t c = 0; c < strong.size(); c++) {
            KeyFrame *nb = strong[c];
            if (!nb || nb == parent || kf->hasChild(nb) || loops.count(nb)) continue;   // already an edge of another kind
            if (nb->isBad() || !(nb->mnId < kf->mnId)) continue;                          // once per pair, from the younger end
            if (sGuarded.count(Graph::ids(kf, nb))) continue;
            graph.add(kf, nb, 0);
        }
    }

    // Step 7's input: every point with the vertex of the keyframe that corrects it (-1: left where it is)
    std::vector<float> vWorld;
    std::vector<int32_t> vRef;
    for (size_t k = 0; k < vpMPs.size(); k++) {
        MapPoint *mp = vpMPs[k];
        const cv::Mat Xw = mp->GetWorldPos();
        for (int c = 0; c < 3; c++) vWorld.push_back(Xw.at<float>(c));
        int32_t ref = -1;
        if (!mp->isBad()) {
            const long unsigned int id = mp->mnCorrectedByKF == pCurKF->mnId ? mp->mnCorrectedReference
                                                                            : mp->GetReferenceKeyFrame()->mnId;
            if (id <= nMaxKFid) ref = vnVertex[id];
        }
        vRef.push_back(ref);
    }

    // Optimize!
    const size_t nVertices = vpVertexKF.size();
    std::vector<double> vSiwOut(8 * nVertices, 0.0);
    std::vector<float> vTiwOut(16 * nVertices, 0.f), vWorldOut(vWorld.size(), 0.f);
    orbx_essgraph_problem P;
    P.nvertices = (int32_t)nVertices; P.nedges = (int32_t)(vEdges.size() / 3); P.npoints = (int32_t)vRef.size();
    P.fix_scale = bFixScale ? 1 : 0;
    P.Scw = vScw8.data(); P.fixed = vFixed.data();
    P.non_corrected = vNonCorrected8.data(); P.has_non_corrected = vHasNonCorrected.data();
    P.edges = vEdges.data(); P.world = vWorld.data(); P.ref = vRef.data();
    P.Siw_out = vSiwOut.data(); P.Tiw_out = vTiwOut.data(); P.world_out = vWorldOut.data();
    orbx_essgraph_result res;
    if (orbx_optimize_essential_graph_batch(host.h, 1, &P, &res) != ORBX_OK) throw std::runtime_error(orbx_last_error());

    unique_lock<mutex> lock(pMap->mMutexMapUpdate);

    // Step 6: Tiw = [R, t / s] into every vertex's keyframe
    for (size_t v = 0; v < nVertices; v++) {
        cv::Mat Tiw(4, 4, CV_32F);
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) Tiw.at<float>(r, c) = vTiwOut[16 * v + 4 * r + c];
        vpVertexKF[v]->SetPose(Tiw);
    }

    // Step 7: the corrected points, then one refresh in place of the per-point UpdateNormalAndDepth
    std::vector<MapPoint *> vpMoved;
    for (size_t k = 0; k < vpMPs.size(); k++) {
        if (vRef[k] < 0) continue;
        cv::Mat Xw(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) Xw.at<float>(c) = vWorldOut[3 * k + c];
        vpMPs[k]->SetWorldPos(Xw);
        vpMoved.push_back(vpMPs[k]);
    }
    MapPoint::RefreshBatch(vpMoved, false, true);
}
