// oracle/ref: a plain C ABI over the reference's own classes, compiled together with the reference's unmodified sources
// (build_ref.py beside this file names them): DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>, DBoW2::BowVector and
// ORB_SLAM2::KeyFrameDatabase.  Nothing here restates what those classes compute; the functions only move data in and out.
// Every function returns 0 on success, -1 after a C++ exception (text in ref_error()) unless stated otherwise.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "KeyFrameDatabase.h"

using DBoW2::BowVector;
using DBoW2::FeatureVector;
typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> RefVocabulary;

namespace {
struct Voc : public RefVocabulary {
    using RefVocabulary::transform;   // the per-feature overload (word, weight, node) is protected in the reference
};
struct Db {
    explicit Db(const Voc &v) : db(v) {}
    ~Db() { for (size_t i = 0; i < kfs.size(); ++i) delete kfs[i]; }
    ORB_SLAM2::KeyFrameDatabase db;
    std::vector<ORB_SLAM2::KeyFrame *> kfs;   // every keyframe ever made; a handle is an index; erased ones keep their fields
};
std::string g_error;
BowVector make_bow(const uint32_t *w, const double *v, int n) {
    BowVector b;
    for (int i = 0; i < n; ++i) b.insert(b.end(), std::make_pair((DBoW2::WordId)w[i], (DBoW2::WordValue)v[i]));
    return b;
}
int put_ids(const std::vector<ORB_SLAM2::KeyFrame *> &c, int64_t *out, int cap, int *n) {
    *n = (int)c.size();
    if ((int)c.size() > cap) { g_error = "output capacity"; return -1; }
    for (size_t i = 0; i < c.size(); ++i) out[i] = (int64_t)c[i]->mnId;
    return 0;
}
}  // namespace

#define REF_TRY try {
#define REF_END } catch (const std::exception &e) { g_error = e.what(); return -1; } \
                  catch (const std::string &e) { g_error = e; return -1; } catch (...) { g_error = "unknown exception"; return -1; } \
                  return 0;

extern "C" {

const char *ref_error() { return g_error.c_str(); }
const char *ref_compiler() { return __VERSION__; }
// 1 when the compiler was allowed to contract a * b + c (the -mfma build), 0 otherwise
int ref_fp_fast_fma() {
#ifdef __FMA__
    return 1;
#else
    return 0;
#endif
}

// ---- vocabulary
int ref_voc_load(const char *path, void **out) {
    REF_TRY
    Voc *v = new Voc();
    if (!v->loadFromTextFile(path) || v->empty()) { delete v; g_error = std::string("loadFromTextFile failed: ") + path; return -1; }
    *out = v;
    REF_END
}
void ref_voc_free(void *v) { delete (Voc *)v; }
int ref_voc_size(const void *v) { return (int)((const Voc *)v)->size(); }
int ref_voc_scoring(const void *v) { return (int)((const Voc *)v)->getScoringType(); }
int ref_voc_weighting(const void *v) { return (int)((const Voc *)v)->getWeightingType(); }

// transform(features, BowVector&, FeatureVector&, levelsup), flattened in map order (capacities: n; fv_begin: n + 2), and
// the per-feature overload.  node_id[i] is preset to 0xFFFFFFFF: the reference does not assign *nid when the descent reaches a
// leaf above level L - levelsup, and the caller sees which features that concerns.
int ref_voc_transform(const void *voc, const uint8_t *desc, int n, int levelsup, uint32_t *word_id, double *weight,
                      uint32_t *node_id, uint32_t *bow_word, double *bow_value, int *n_bow, uint32_t *fv_node, int32_t *fv_begin,
                      uint32_t *fv_index, int *n_fv_nodes) {
    REF_TRY
    const Voc *v = (const Voc *)voc;
    std::vector<cv::Mat> feats((size_t)n);
    for (int i = 0; i < n; ++i) {
        feats[i].create(1, 32, CV_8U);
        std::memcpy(feats[i].ptr<unsigned char>(), desc + 32 * (size_t)i, 32);
    }
    for (int i = 0; i < n; ++i) {
        DBoW2::WordId id = 0; DBoW2::WordValue w = 0; DBoW2::NodeId nid = 0xFFFFFFFFu;
        v->transform(feats[i], id, w, &nid, levelsup);
        word_id[i] = id; weight[i] = w; node_id[i] = nid;
    }
    BowVector bv; FeatureVector fv;
    v->transform(feats, bv, fv, levelsup);
    int nb = 0;
    for (BowVector::const_iterator it = bv.begin(); it != bv.end(); ++it, ++nb) { bow_word[nb] = it->first; bow_value[nb] = it->second; }
    *n_bow = nb;
    int nn = 0, pos = 0;
    fv_begin[0] = 0;
    for (FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        fv_node[nn] = it->first;
        for (size_t k = 0; k < it->second.size(); ++k) fv_index[pos++] = it->second[k];
        fv_begin[++nn] = pos;
    }
    *n_fv_nodes = nn;
    REF_END
}

int ref_voc_score(const void *voc, const uint32_t *w1, const double *v1, int n1, const uint32_t *w2, const double *v2, int n2,
                  double *out) {
    REF_TRY
    *out = ((const Voc *)voc)->score(make_bow(w1, v1, n1), make_bow(w2, v2, n2));
    REF_END
}

// BowVector::normalize(norm_type): 0 = DBoW2::L1, 1 = DBoW2::L2; values in place
int ref_bow_normalize(const uint32_t *w, double *v, int n, int norm_type) {
    REF_TRY
    BowVector b = make_bow(w, v, n);
    b.normalize(norm_type == 0 ? DBoW2::L1 : DBoW2::L2);
    int i = 0;
    for (BowVector::const_iterator it = b.begin(); it != b.end(); ++it) v[i++] = it->second;
    REF_END
}

// ---- keyframe database
int ref_db_create(const void *voc, void **out) {
    REF_TRY
    *out = new Db(*(const Voc *)voc);
    REF_END
}
void ref_db_free(void *db) { delete (Db *)db; }
// a new KeyFrame (not yet in the database); returns its handle, or -1
int ref_kf_new(void *db, int64_t id, const uint32_t *w, const double *v, int n) {
    try {
        Db *d = (Db *)db;
        ORB_SLAM2::KeyFrame *kf = new ORB_SLAM2::KeyFrame((long unsigned int)id);
        kf->mBowVec = make_bow(w, v, n);
        d->kfs.push_back(kf);
        return (int)d->kfs.size() - 1;
    } catch (...) { g_error = "ref_kf_new"; return -1; }
}
int ref_db_add(void *db, int kf) { REF_TRY Db *d = (Db *)db; d->db.add(d->kfs.at(kf)); REF_END }
int ref_db_erase(void *db, int kf) { REF_TRY Db *d = (Db *)db; d->db.erase(d->kfs.at(kf)); REF_END }
int ref_db_clear(void *db) { REF_TRY ((Db *)db)->db.clear(); REF_END }
int ref_kf_set_connected(void *db, int kf, const int32_t *handles, int n) {
    REF_TRY
    Db *d = (Db *)db;
    std::set<ORB_SLAM2::KeyFrame *> s;
    for (int i = 0; i < n; ++i) s.insert(d->kfs.at(handles[i]));
    d->kfs.at(kf)->connected = s;
    REF_END
}
// ordered covisibility lists of nkf keyframes at once: list i = flat[begin[i] .. begin[i + 1])
int ref_kf_set_ordered(void *db, int nkf, const int32_t *kf, const int32_t *begin, const int32_t *flat) {
    REF_TRY
    Db *d = (Db *)db;
    for (int i = 0; i < nkf; ++i) {
        std::vector<ORB_SLAM2::KeyFrame *> o;
        for (int k = begin[i]; k < begin[i + 1]; ++k) o.push_back(d->kfs.at(flat[k]));
        d->kfs.at(kf[i])->ordered = o;
    }
    REF_END
}
int ref_db_detect_loop(void *db, int kf, float min_score, int64_t *out, int cap, int *n) {
    REF_TRY
    Db *d = (Db *)db;
    if (put_ids(d->db.DetectLoopCandidates(d->kfs.at(kf), min_score), out, cap, n)) return -1;
    REF_END
}
int ref_db_detect_reloc(void *db, int64_t frame_id, const uint32_t *w, const double *v, int nw, int64_t *out, int cap, int *n) {
    REF_TRY
    Db *d = (Db *)db;
    ORB_SLAM2::Frame F;
    F.mnId = (long unsigned int)frame_id;
    F.mBowVec = make_bow(w, v, nw);
    if (put_ids(d->db.DetectRelocalizationCandidates(&F), out, cap, n)) return -1;
    REF_END
}
// the six query fields: [0] relocalisation form, [1] loop form
int ref_kf_fields(void *db, int kf, int64_t *mark, int32_t *words, float *score) {
    REF_TRY
    const ORB_SLAM2::KeyFrame *k = ((Db *)db)->kfs.at(kf);
    mark[0] = (int64_t)k->mnRelocQuery; words[0] = k->mnRelocWords; score[0] = k->mRelocScore;
    mark[1] = (int64_t)k->mnLoopQuery; words[1] = k->mnLoopWords; score[1] = k->mLoopScore;
    REF_END
}

}  // extern "C"
