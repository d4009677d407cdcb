"""Independent restatement of ORB_SLAM2::KeyFrameDatabase (reference src/KeyFrameDatabase.cc:56-411) and of DBoW2's six
scoring functions (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-315), list by list and field by field, with the F8 rule of
DESIGN.md section 2.

The reference keeps the query marks, word counts and scores in the KeyFrames; so does the model (class KeyFrame).  Scores are
Python floats (IEEE double) narrowed to numpy float32 where the reference narrows them (`float si = mpVoc->score(...)`);
accScore and every comparison of steps 4-5 are float32.  Results are compared as bit patterns.

The model follows the source text; tests/test_ref_dbow2.py pins it to the source itself, compiled with g++ under two flag sets
behind stand-ins for cv::Mat, KeyFrame and Frame (oracle/ref/): scores, candidates, list order and the per-keyframe fields
equal the compiled code bit for bit, with `fma_mode=False` against -O3 -ffp-contract=off and `fma_mode=True` against -O3 -mfma.
The fused multiply-add of `score += vi * wi` under the default fp_mode is therefore what GCC emits, not an
assumption.  The stand-in KeyFrame starts the two scores at 0.0f, the value a never-written score reads as here."""
import math
from fractions import Fraction
import numpy as np

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
LOG_EPS = math.log(2.220446049250313e-16)   # GeneralScoring::LOG_EPS = log(DBL_EPSILON)


def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then the correctly rounded conversion)"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c    # the sign of an exact zero follows the IEEE rule of the unfused form here
    return float(r)


def _muladd(score, a, b, fma_mode):
    return fma(a, b, score) if fma_mode else score + a * b


def score(scoring, v1, v2, fma_mode=True):
    """GeneralScoring::score(v1, v2); v = (ascending word ids, values).  The merge walk with lower_bound of the reference."""
    w1, x1 = v1
    w2, x2 = v2
    n1, n2 = len(w1), len(w2)
    i = j = 0
    s = 0.0

    def lower_bound(w, n, start, key):   # std::map::lower_bound: first element with word >= key
        k = start
        while k < n and w[k] < key:
            k += 1
        return k

    while i < n1 and j < n2:
        vi, wi = float(x1[i]), float(x2[j])
        if w1[i] == w2[j]:
            if scoring == L1_NORM:
                s += abs(vi - wi) - abs(vi) - abs(wi)
            elif scoring in (L2_NORM, DOT_PRODUCT):
                s = _muladd(s, vi, wi, fma_mode)
            elif scoring == CHI_SQUARE:
                if vi + wi != 0.0:
                    s += vi * wi / (vi + wi)
            elif scoring == KL:
                if vi != 0 and wi != 0:
                    s = _muladd(s, vi, math.log(vi / wi), fma_mode)
            else:
                s += math.sqrt(vi * wi)
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            if scoring == KL:
                s = _muladd(s, vi, math.log(vi) - LOG_EPS, fma_mode)
                i += 1
            else:
                i = lower_bound(w1, n1, i, w2[j])
        else:
            j = lower_bound(w2, n2, j, w1[i])
    if scoring == L1_NORM:
        return -s / 2.0
    if scoring == L2_NORM:
        return 1.0 if s >= 1 else 1.0 - math.sqrt(1.0 - s)
    if scoring == CHI_SQUARE:
        return 2.0 * s
    if scoring == KL:
        while i < n1:
            if float(x1[i]) != 0:
                s = _muladd(s, float(x1[i]), math.log(float(x1[i])) - LOG_EPS, fma_mode)
            i += 1
    return s


class KeyFrame:
    """the fields of ORB_SLAM2::KeyFrame the database touches (KeyFrame.cc:53-56: marks and word counts start at 0, the two
    scores are not initialised: None here)"""

    def __init__(self, mnId, bow):
        self.mnId = int(mnId)
        self.mBowVec = (np.asarray(bow[0], np.uint32), np.asarray(bow[1], np.float64))
        self.mnLoopQuery = 0
        self.mnLoopWords = 0
        self.mLoopScore = None
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = None
        self.connected = []      # GetConnectedKeyFrames()
        self.best_covis = []     # GetBestCovisibilityKeyFrames(10)

    def state(self, loop):
        m, w, s = (self.mnLoopQuery, self.mnLoopWords, self.mLoopScore) if loop else \
            (self.mnRelocQuery, self.mnRelocWords, self.mRelocScore)
        return m, w, np.float32(0) if s is None else s, int(s is not None)


class Result:
    def __init__(self):
        self.sharing = []            # lKFsSharingWords
        self.min_common = 0          # minCommonWords
        self.score_and_match = []    # lScoreAndMatch: (float32 si, KeyFrame)
        self.candidates = []         # vpLoopCandidates / vpRelocCandidates
        self.nscores = 0
        self.stale_reads = 0         # F8: a score an earlier query wrote, read for a neighbour this query did not score
        self.unscored_reads = 0      # F8: a score nothing ever wrote (read as 0.0f)
        self.rejected_min_score = 0
        self.connected_met = 0


def min_common_words(max_common):
    """`int minCommonWords = maxCommonWords * 0.8f;`: int -> float, float product, truncation"""
    return int(np.float32(max_common) * np.float32(0.8))


class KeyFrameDatabase:
    def __init__(self, scoring=L1_NORM, fma_mode=True):
        self.scoring, self.fma_mode = scoring, fma_mode
        self.mvInvertedFile = {}     # word id -> list of KeyFrame, in add order

    def add(self, pKF):
        for w in pKF.mBowVec[0]:
            self.mvInvertedFile.setdefault(int(w), []).append(pKF)

    def erase(self, pKF):
        for w in pKF.mBowVec[0]:
            lKFs = self.mvInvertedFile.get(int(w), [])
            for k, kf in enumerate(lKFs):
                if kf is pKF:
                    del lKFs[k]
                    break

    def clear(self):
        self.mvInvertedFile = {}

    def vocabulary_score(self, a, b):
        return score(self.scoring, a, b, self.fma_mode)

    def _read_score(self, value, scored_now, res):
        if value is None:
            res.unscored_reads += 1
            return np.float32(0)
        if not scored_now:
            res.stale_reads += 1
        return value

    def DetectLoopCandidates(self, pKF, minScore):
        minScore = np.float32(minScore)
        res = Result()
        spConnectedKeyFrames = set(id(k) for k in pKF.connected)
        lKFsSharingWords = res.sharing
        for w in pKF.mBowVec[0]:
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnLoopQuery != pKF.mnId:
                    pKFi.mnLoopWords = 0
                    if id(pKFi) not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = pKF.mnId
                        lKFsSharingWords.append(pKFi)
                    else:
                        res.connected_met += 1
                pKFi.mnLoopWords += 1
        if not lKFsSharingWords:
            return res
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnLoopWords > maxCommonWords:
                maxCommonWords = k.mnLoopWords
        minCommonWords = res.min_common = min_common_words(maxCommonWords)
        scored = set()
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                res.nscores += 1
                si = np.float32(self.vocabulary_score(pKF.mBowVec, pKFi.mBowVec))
                pKFi.mLoopScore = si
                scored.add(id(pKFi))
                if si >= minScore:
                    res.score_and_match.append((si, pKFi))
                else:
                    res.rejected_min_score += 1
        if not res.score_and_match:
            return res
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in res.score_and_match:
            bestScore = accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.best_covis:
                if pKF2.mnLoopQuery == pKF.mnId and pKF2.mnLoopWords > minCommonWords:
                    s2 = self._read_score(pKF2.mLoopScore, id(pKF2) in scored, res)
                    accScore = np.float32(accScore + s2)
                    if s2 > bestScore:
                        pBestKF, bestScore = pKF2, s2
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        self._retain(lAccScoreAndMatch, bestAccScore, res)
        return res

    def DetectRelocalizationCandidates(self, F):
        """F: anything with mnId and mBowVec"""
        res = Result()
        lKFsSharingWords = res.sharing
        for w in F.mBowVec[0]:
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:
            return res
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = res.min_common = min_common_words(maxCommonWords)
        scored = set()
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                res.nscores += 1
                si = np.float32(self.vocabulary_score(F.mBowVec, pKFi.mBowVec))
                pKFi.mRelocScore = si
                scored.add(id(pKFi))
                res.score_and_match.append((si, pKFi))
        if not res.score_and_match:
            return res
        lAccScoreAndMatch = []
        bestAccScore = np.float32(0)
        for si, pKFi in res.score_and_match:
            bestScore = accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.best_covis:
                if pKF2.mnRelocQuery != F.mnId:
                    continue
                s2 = self._read_score(pKF2.mRelocScore, id(pKF2) in scored, res)   # F8: no word-count guard here
                accScore = np.float32(accScore + s2)
                if s2 > bestScore:
                    pBestKF, bestScore = pKF2, s2
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        self._retain(lAccScoreAndMatch, bestAccScore, res)
        return res

    @staticmethod
    def _retain(lAccScoreAndMatch, bestAccScore, res):
        minScoreToRetain = np.float32(np.float32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        for acc, pKFi in lAccScoreAndMatch:
            if acc > minScoreToRetain:
                if id(pKFi) not in spAlreadyAddedKF:
                    res.candidates.append(pKFi)
                    spAlreadyAddedKF.add(id(pKFi))


class Frame:
    def __init__(self, mnId, bow):
        self.mnId = int(mnId)
        self.mBowVec = (np.asarray(bow[0], np.uint32), np.asarray(bow[1], np.float64))
