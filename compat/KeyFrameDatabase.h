// compat/KeyFrameDatabase.h -- drop-in replacement of the reference's include/KeyFrameDatabase.h + src/KeyFrameDatabase.cc.
//
// Same namespace, class name and public surface (reference include/KeyFrameDatabase.h:44-85: the constructor from the
// vocabulary, add, erase, clear, DetectLoopCandidates, DetectRelocalizationCandidates), so System.cc:98, Tracking.cc:2255 / 2528,
// LoopClosing.cc:177-371 and KeyFrame.cc:845 compile unchanged.  The BowVectors of the keyframes live in an orbx_kfdb of
// liborbx.so (include/orbx.h); every method marshals what the reference's reads -- mBowVec, GetConnectedKeyFrames(),
// GetBestCovisibilityKeyFrames(10), evaluated at the moment the reference evaluates them -- calls the library, and writes
// mnLoopQuery / mnLoopWords / mLoopScore and mnRelocQuery / mnRelocWords / mRelocScore of every keyframe the query touched back
// into the KeyFrame, so that other code of the reference sees the state it would have seen.  One difference, stated in
// a score the reference would read uninitialised is 0.0f here (UnscoredReads() counts those reads of the
// last query); a keyframe's score member is only written once a query has scored it.
//
// The database works on the device of the orbx_handle it is given: SetHandle(extractor->handle()) before the first add shares
// the extractor's; without it the database creates a handle of its own on the current device with the first use.
// Needs the ORB-SLAM2 tree (KeyFrame.h, Frame.h, ORBVocabulary.h).  This repository's tests build and run it against stand-ins
// of those (tests/compat_kfdb/); the maintainer's build inside an ORB-SLAM2 tree remains the final check.
// Remove src/KeyFrameDatabase.cc from the library's sources.
#ifndef KEYFRAMEDATABASE_H
#define KEYFRAMEDATABASE_H

#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <vector>

#include "KeyFrame.h"
#include "Frame.h"
#include "ORBVocabulary.h"
#include "orbx.h"

namespace ORB_SLAM2 {

class KeyFrame;
class Frame;

class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary &voc) : mpVoc(&voc) {}
    ~KeyFrameDatabase() {
        if (db_) orbx_kfdb_destroy(db_);
        if (own_) orbx_destroy(own_);
    }
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;

    // not in the reference: the handle whose device holds the database (before the first add)
    void SetHandle(orbx_handle *h) {
        std::unique_lock<std::mutex> lock(mMutex);
        if (db_) throw std::logic_error("KeyFrameDatabase::SetHandle after the first use");
        h_ = h;
    }
    int UnscoredReads() const { return unscored_reads_; }   // F8 reads of the last Detect* call

    // src/KeyFrameDatabase.cc:56-62
    void add(KeyFrame *pKF) {
        std::unique_lock<std::mutex> lock(mMutex);
        Flatten(pKF->mBowVec);
        Check(orbx_kfdb_add(Db(), (int64_t)pKF->mnId, w_.data(), v_.data(), (int)w_.size()));
        kfs_[(int64_t)pKF->mnId] = pKF;
    }
    // :70-88.  Like the reference, erasing a keyframe that was never added changes nothing.
    void erase(KeyFrame *pKF) {
        std::unique_lock<std::mutex> lock(mMutex);
        std::map<int64_t, KeyFrame *>::iterator it = kfs_.find((int64_t)pKF->mnId);
        if (it == kfs_.end() || it->second != pKF) return;
        Check(orbx_kfdb_erase(Db(), (int64_t)pKF->mnId));
        kfs_.erase(it);
    }
    // :94-100
    void clear() {
        std::unique_lock<std::mutex> lock(mMutex);
        if (db_) Check(orbx_kfdb_clear(db_));
        kfs_.clear();
    }

    // :114-263, caller LoopClosing::DetectLoop (src/LoopClosing.cc:209)
    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *pKF, float minScore) {
        const std::set<KeyFrame *> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<int64_t> connected;
        for (std::set<KeyFrame *>::const_iterator it = spConnectedKeyFrames.begin(); it != spConnectedKeyFrames.end(); ++it)
            if (Known(*it)) connected.push_back((int64_t)(*it)->mnId);
        Flatten(pKF->mBowVec);
        int32_t n_matches = 0, min_common = 0;
        Check(orbx_kfdb_query_loop(Db(), (int64_t)pKF->mnId, w_.data(), v_.data(), (int)w_.size(), connected.data(),
                                   (int)connected.size(), minScore, &n_matches, &min_common));
        return Groups(n_matches, true);
    }

    // :274-411, caller Tracking::Relocalization (src/Tracking.cc:2255)
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F) {
        std::unique_lock<std::mutex> lock(mMutex);
        Flatten(F->mBowVec);
        const int64_t id = (int64_t)F->mnId;
        const int32_t q_begin[2] = {0, (int32_t)w_.size()};
        int32_t n_matches = 0, min_common = 0;
        Check(orbx_kfdb_query_reloc(Db(), 1, &id, q_begin, w_.data(), v_.data(), &n_matches, &min_common));
        return Groups(n_matches, false);
    }

protected:
    const ORBVocabulary *mpVoc;
    std::mutex mMutex;

private:
    static void Check(orbx_status s) {
        if (s != ORBX_OK) throw std::runtime_error(orbx_last_error());
    }
    orbx_kfdb *Db() {
        if (!db_) {
            if (!h_) {
                orbx_params p;
                orbx_default_params(&p);
                Check(orbx_create(&p, &own_));
                h_ = own_;
            }
            Check(orbx_kfdb_create(h_, (int)mpVoc->getScoringType(), &db_));
        }
        return db_;
    }
    bool Known(KeyFrame *pKF) const {
        std::map<int64_t, KeyFrame *>::const_iterator it = kfs_.find((int64_t)pKF->mnId);
        return it != kfs_.end() && it->second == pKF;
    }
    template <class BowVector> void Flatten(const BowVector &bow) {   // std::map order = ascending word id
        w_.clear(); v_.clear();
        for (typename BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) {
            w_.push_back((uint32_t)it->first);
            v_.push_back((double)it->second);
        }
    }
    // steps 4-5 and the write-back.  GetBestCovisibilityKeyFrames(10) is the caller's state and is evaluated here, per entry of
    // lScoreAndMatch, where the reference evaluates it; the query fields of the touched keyframes are written once at the end.
    std::vector<KeyFrame *> Groups(int n_matches, bool loop) {
        unscored_reads_ = 0;
        std::vector<int64_t> ids((size_t)n_matches + 1), neigh;
        std::vector<float> scores((size_t)n_matches + 1);
        std::vector<int32_t> begin(1, 0);
        int n = 0;
        Check(orbx_kfdb_query_matches(db_, 0, ids.data(), scores.data(), n_matches, &n));
        for (int i = 0; i < n; ++i) {
            const std::vector<KeyFrame *> vpNeighs = kfs_[ids[i]]->GetBestCovisibilityKeyFrames(10);
            for (size_t k = 0; k < vpNeighs.size(); ++k)
                if (Known(vpNeighs[k])) neigh.push_back((int64_t)vpNeighs[k]->mnId);
            begin.push_back((int32_t)neigh.size());
        }
        std::vector<int64_t> cand((size_t)n + 1);
        int nc = 0;
        Check(orbx_kfdb_select_groups(db_, 0, begin.data(), neigh.data(), cand.data(), n, &nc, &unscored_reads_));
        int nt = 0;
        orbx_kfdb_query_touched(db_, 0, NULL, 0, &nt);
        std::vector<int64_t> touched((size_t)nt + 1);
        Check(orbx_kfdb_query_touched(db_, 0, touched.data(), nt, &nt));
        for (int i = 0; i < nt; ++i) {
            KeyFrame *k = kfs_[touched[i]];
            int64_t mark = 0; int32_t words = 0; float score = 0.f; int valid = 0;
            Check(orbx_kfdb_state(db_, touched[i], loop ? 1 : 0, &mark, &words, &score, &valid));
            if (loop) { k->mnLoopQuery = (long unsigned int)mark; k->mnLoopWords = words; if (valid) k->mLoopScore = score; }
            else { k->mnRelocQuery = (long unsigned int)mark; k->mnRelocWords = words; if (valid) k->mRelocScore = score; }
        }
        std::vector<KeyFrame *> out;
        out.reserve((size_t)nc);
        for (int i = 0; i < nc; ++i) out.push_back(kfs_[cand[i]]);
        return out;
    }

    orbx_handle *h_ = NULL, *own_ = NULL;
    orbx_kfdb *db_ = NULL;
    std::map<int64_t, KeyFrame *> kfs_;
    std::vector<uint32_t> w_;
    std::vector<double> v_;
    int unscored_reads_ = 0;
};

}  // namespace ORB_SLAM2

#endif  // KEYFRAMEDATABASE_H
