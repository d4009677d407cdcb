// tests/compat_kfdb: extern "C" entry points through which tests/test_kfdb.py drives compat/KeyFrameDatabase.h against the
// stand-ins of this directory.  One world at a time: a database, its keyframes by id, their covisibility lists.
// Every call returns 0, or -1 after any C++ exception, whose text kf_error() then returns.
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include "KeyFrameDatabase.h"

using namespace ORB_SLAM2;

namespace {
std::string g_error;
orbx_handle *g_h = nullptr;
std::unique_ptr<ORBVocabulary> g_voc;
std::unique_ptr<KeyFrameDatabase> g_db;
std::map<long, std::unique_ptr<KeyFrame>> g_kfs;   // erased keyframes stay alive, as bad keyframes do in the map

template <class F> int guarded(F &&f) {
    try { f(); return 0; }
    catch (const std::exception &e) { g_error = e.what(); }
    catch (...) { g_error = "unknown exception"; }
    return -1;
}
void fill(DBoW2::BowVector &b, const uint32_t *w, const double *v, int n) {
    b.clear();
    for (int i = 0; i < n; ++i) b[w[i]] = v[i];
}
int copy_out(const std::vector<KeyFrame *> &c, long *out, int cap) {
    if ((int)c.size() > cap) throw std::runtime_error("candidate buffer too small");
    for (size_t i = 0; i < c.size(); ++i) out[i] = (long)c[i]->mnId;
    return (int)c.size();
}
}  // namespace

extern "C" {
const char *kf_error() { return g_error.c_str(); }

// device = -2: host-only handle; otherwise the device ordinal
int kf_reset(int device, int scoring) {
    return guarded([&] {
        g_db.reset(); g_kfs.clear(); g_voc.reset();
        if (g_h) { orbx_destroy(g_h); g_h = nullptr; }
        orbx_params p;
        orbx_default_params(&p);
        p.device = device;
        if (orbx_create(&p, &g_h) != ORBX_OK) throw std::runtime_error(orbx_last_error());
        g_voc.reset(new ORBVocabulary((DBoW2::ScoringType)scoring));
        g_db.reset(new KeyFrameDatabase(*g_voc));
        g_db->SetHandle(g_h);
    });
}
int kf_new(long id, const uint32_t *w, const double *v, int n) {
    return guarded([&] {
        g_kfs[id].reset(new KeyFrame((long unsigned int)id));
        fill(g_kfs[id]->mBowVec, w, v, n);
    });
}
int kf_add(long id) { return guarded([&] { g_db->add(g_kfs.at(id).get()); }); }
int kf_erase(long id) { return guarded([&] { g_db->erase(g_kfs.at(id).get()); }); }
int kf_clear() { return guarded([&] { g_db->clear(); }); }
int kf_set_graph(long id, const long *connected, int nc, const long *ordered, int no) {
    return guarded([&] {
        KeyFrame *k = g_kfs.at(id).get();
        k->connected.clear(); k->ordered.clear();
        for (int i = 0; i < nc; ++i) k->connected.insert(g_kfs.at(connected[i]).get());
        for (int i = 0; i < no; ++i) k->ordered.push_back(g_kfs.at(ordered[i]).get());
    });
}
int kf_reloc(long frame_id, const uint32_t *w, const double *v, int n, long *out, int cap, int *nout, int *unscored) {
    return guarded([&] {
        Frame F;
        F.mnId = (long unsigned int)frame_id;
        fill(F.mBowVec, w, v, n);
        *nout = copy_out(g_db->DetectRelocalizationCandidates(&F), out, cap);
        *unscored = g_db->UnscoredReads();
    });
}
int kf_loop(long id, float min_score, long *out, int cap, int *nout, int *unscored) {
    return guarded([&] {
        *nout = copy_out(g_db->DetectLoopCandidates(g_kfs.at(id).get(), min_score), out, cap);
        *unscored = g_db->UnscoredReads();
    });
}
// the six query fields as the KeyFrame object holds them (what other code of the reference would read)
int kf_fields(long id, long *marks2, int *words2, float *scores2) {
    return guarded([&] {
        const KeyFrame *k = g_kfs.at(id).get();
        marks2[0] = (long)k->mnRelocQuery; marks2[1] = (long)k->mnLoopQuery;
        words2[0] = k->mnRelocWords; words2[1] = k->mnLoopWords;
        scores2[0] = k->mRelocScore; scores2[1] = k->mLoopScore;
    });
}
}
