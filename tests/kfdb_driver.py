"""Plays one seeded sequence of add / erase / relocalisation query / loop query / score calls on the model (kfdb_model.py) and on
a library database at the same time and compares everything observable after every call (tests/test_kfdb.py).

Input recipe: a trajectory through `places`; the words of a place come from a window of a permuted vocabulary that overlaps
the windows of the adjacent places by half, plus a fifth drawn uniformly.  GetBestCovisibilityKeyFrames(10) of an entry = the
live entries of the same and the adjacent places nearest in add order; GetConnectedKeyFrames() of a loop query = the recently
added entries of those places (so that an old visit of the same place is a loop candidate)."""
import numpy as np
import kfdb_model as M


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


class World:
    def __init__(self, seed, *, places=12, words=48, vocab=4000, scoring=M.L1_NORM, fma_mode=True):
        self.rng = np.random.default_rng(seed)
        self.places, self.words, self.vocab = places, words, vocab
        self.perm = self.rng.permutation(vocab)
        self.window = 2 * words
        assert (places + 1) * words + self.window <= vocab
        self.model = M.KeyFrameDatabase(scoring, fma_mode)
        self.kfs = {}          # id -> model KeyFrame (live entries)
        self.place_of = {}
        self.order = []        # live ids in add order
        self.next_kf, self.next_frame = 1, 1
        self.covis = None      # hand-made cases: id -> neighbour ids instead of the place rule
        self.stats = dict(reloc=0, reloc_with_candidates=0, stale=0, unscored=0, rejected_min_score=0, connected_met=0, loop=0,
                          scored=0, sharers=0)

    def draw(self, place, nw=None):
        nw = self.words if nw is None else nw
        nu = max(1, nw // 5) if nw > 1 else 0
        pool = self.perm[place * self.words: place * self.words + self.window]
        a = self.rng.choice(pool, size=min(nw - nu, len(pool)), replace=False)
        b = self.rng.integers(0, self.vocab, size=nu)
        w = np.unique(np.concatenate([a, b]).astype(np.uint32))
        v = self.rng.random(len(w)) + 0.05
        return w, (v / v.sum()).astype(np.float64)

    def near(self, place, kf_id=None):
        return [i for i in self.order if abs(self.place_of[i] - place) <= 1 and i != kf_id]

    def set_covisibility(self):
        for i, kf in self.kfs.items():
            if self.covis is not None:
                kf.best_covis = [self.kfs[j] for j in self.covis.get(i, []) if j in self.kfs]
                continue
            cand = self.near(self.place_of[i], i)
            cand.sort(key=lambda j: (abs(j - i), j))
            kf.best_covis = [self.kfs[j] for j in cand[:10]]


class Checked:
    """the model and one library database in lockstep"""

    def __init__(self, world, db):
        self.w, self.db = world, db

    # ---- mutations
    def add(self, place, nw=None, kf_id=None, bow=None):
        w = self.w
        if kf_id is None:
            kf_id = w.next_kf
            w.next_kf += 1
        bow = w.draw(place, nw) if bow is None else bow
        kf = M.KeyFrame(kf_id, bow)
        w.model.add(kf)
        w.kfs[kf_id] = kf; w.place_of[kf_id] = place; w.order.append(kf_id)
        self.db.add(kf_id, bow)
        return kf_id

    def erase(self, kf_id):
        w = self.w
        w.model.erase(w.kfs.pop(kf_id))
        w.order.remove(kf_id); del w.place_of[kf_id]
        self.db.erase(kf_id)

    # ---- comparisons
    def check_state(self):
        for i, kf in self.w.kfs.items():
            for loop in (False, True):
                m, n, s, ok = self.db.state(i, loop)
                em, en, es, eok = kf.state(loop)
                assert (m, n, ok) == (em, en, eok), (i, loop, (m, n, ok), (em, en, eok))
                assert bits(s) == bits(es), (i, loop, s, es)

    def _check_query(self, res, got, q, groups=True):
        ids, sc, mc = got
        exp_ids = [kf.mnId for _, kf in res.score_and_match]
        assert list(ids) == exp_ids, (list(ids), exp_ids)
        assert np.array_equal(bits(sc), bits([s for s, _ in res.score_and_match]))
        if res.sharing:
            assert mc == res.min_common, (mc, res.min_common)
        if groups:
            neigh = [[k.mnId for k in self.w.kfs[i].best_covis] for i in exp_ids]
            cand, unscored = self.db.select_groups(q, neigh)
            assert list(cand) == [k.mnId for k in res.candidates], (list(cand), [k.mnId for k in res.candidates])
            assert unscored == res.unscored_reads, (unscored, res.unscored_reads)

    def _count(self, res, reloc):
        st = self.w.stats
        st["stale"] += res.stale_reads; st["unscored"] += res.unscored_reads
        st["rejected_min_score"] += res.rejected_min_score; st["connected_met"] += res.connected_met
        st["scored"] += res.nscores; st["sharers"] += len(res.sharing)
        if reloc:
            st["reloc"] += 1; st["reloc_with_candidates"] += bool(res.candidates)
        else:
            st["loop"] += 1

    # ---- queries
    def reloc(self, places, frame_ids=None, state=True):
        """len(places) frames in ONE library call, as if run one after the other"""
        w = self.w
        w.set_covisibility()
        frames = []
        for k, p in enumerate(places):
            fid = w.next_frame if frame_ids is None else frame_ids[k]
            if frame_ids is None:
                w.next_frame += 1
            frames.append(M.Frame(fid, w.draw(p) if not isinstance(p, tuple) else p))
        got = self.db.query_reloc([f.mnId for f in frames], [f.mBowVec for f in frames])
        out = []
        for q, f in enumerate(frames):
            res = w.model.DetectRelocalizationCandidates(f)
            self._count(res, True)
            self._check_query(res, got[q], q)
            out.append(res)
        if state:
            self.check_state()
        return out

    def loop(self, place, *, recent=6, same_place=False, min_score=None, kf_id=None, bow=None, add_after=True, connected=None):
        w = self.w
        w.set_covisibility()
        if kf_id is None:
            kf_id = w.next_kf
            w.next_kf += 1
        bow = w.draw(place) if bow is None else bow
        cur = M.KeyFrame(kf_id, bow)
        if connected is None:
            connected = [i for i in w.near(place) if not same_place or w.place_of[i] == place][-recent:]
        cur.connected = [w.kfs[i] for i in connected]
        if min_score is None:     # LoopClosing::DetectLoop (src/LoopClosing.cc:143-157): the lowest score among the connected
            min_score = np.float32(1)
            lib_scores = self.db.score_entries(bow, connected)
            for k, i in enumerate(connected):
                s = w.model.vocabulary_score(bow, w.kfs[i].mBowVec)
                assert np.float64(s).view(np.uint64) == lib_scores[k:k + 1].view(np.uint64)[0], (i, s, lib_scores[k])
                if np.float32(s) < min_score:
                    min_score = np.float32(s)
        got = self.db.query_loop(kf_id, bow, list(connected) + [10 ** 9], min_score)   # an id outside the database is ignored
        res = w.model.DetectLoopCandidates(cur, min_score)
        self._count(res, False)
        self._check_query(res, got, 0)
        self.check_state()
        if add_after:              # LoopClosing adds the keyframe after the query (:118, :132, :181)
            self.add(place, kf_id=kf_id, bow=bow)
        return res


def build_map(c, laps=2, per_place=3):
    """a trajectory that visits every place `laps` times: later visits see the earlier ones as loop / relocalisation candidates"""
    for _ in range(laps):
        for p in range(c.w.places):
            for _ in range(per_place):
                c.add(p)


def play(c, steps, seed):
    """a mixed seeded sequence; returns the model-side statistics the tests assert on before comparing anything"""
    rng = np.random.default_rng(seed)
    w = c.w
    build_map(c)
    for step in range(steps):
        r = rng.random()
        p = int(rng.integers(0, w.places))
        if r < 0.40:
            c.reloc([p])
        elif r < 0.55:
            c.reloc([int(x) for x in rng.integers(0, w.places, size=int(rng.integers(2, 6)))])
        elif r < 0.80:
            c.loop(p, same_place=bool(rng.integers(0, 2)), recent=int(rng.integers(2, 7)))
        elif r < 0.90 and len(w.order) > 20:
            c.erase(int(rng.choice(w.order)))
            c.check_state()
        else:
            c.add(p)
            c.check_state()
    return w.stats


def assert_not_vacuous(st):
    assert st["reloc"] > 0 and st["reloc_with_candidates"] == st["reloc"], st   # every relocalisation query returns a candidate
    assert st["stale"] >= 1 and st["unscored"] >= 1, st
    assert st["loop"] > 0 and st["rejected_min_score"] >= 1 and st["connected_met"] >= 1, st
