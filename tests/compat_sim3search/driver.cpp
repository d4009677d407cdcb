// tests/compat_sim3search: the entry points of tests/compat_runtime/harness.cpp (included as it stands, so that its scene is this
// translation unit's scene) plus the two that tests/test_compat_sim3search.py compares: ORBmatcher::SearchBySim3Batch of
// compat/ORBmatcher.h and the loop of single SearchBySim3 calls it replaces.  Built with -DCS_HOST_HANDLE the batch runs on a
// host-only handle (the library's host path; the single call needs a device and is not called then).
#ifdef CS_HOST_HANDLE
struct orbx_handle;
static orbx_handle *cs_host_handle();
#define ORBX_SIM3SEARCH_HANDLE cs_host_handle()
#endif
#define ORBX_SIM3SEARCH_BATCH_MIN 1
#include "../compat_runtime/harness.cpp"

#ifdef CS_HOST_HANDLE
static orbx_handle *cs_host_handle() {
    static orbx_handle *h = NULL;
    if (!h) {
        orbx_params p;
        orbx_default_params(&p);
        p.device = -2;
#ifdef ORBX_COMPAT_FP_MODE
        p.fp_mode = ORBX_COMPAT_FP_MODE;
#endif
        if (orbx_create(&p, &h) != ORBX_OK) throw std::runtime_error(orbx_last_error());
    }
    return h;
}
#endif

extern "C" {
// matches: K rows of N1 entries, in / out (MapPoint ids, -1 = NULL); R12s 9 per candidate, t12s 3 per candidate.
// batch != 0: one SearchBySim3Batch call; batch == 0: the loop of SearchBySim3 calls.
int cs_search_by_sim3(int kf1, const int *kfs, int K, int *matches, const float *s12s, const float *R12s, const float *t12s, float th,
                      int batch, int *counts) {
    return Guard([&] {
        ORBmatcher m(0.75f, true);
        const int N1 = KF(kf1)->N;
        std::vector<KeyFrame *> v2((size_t)K);
        std::vector<std::vector<MapPoint *> > vv((size_t)K);
        std::vector<float> s((size_t)K);
        std::vector<cv::Mat> R, t;
        for (int k = 0; k < K; ++k) {
            v2[k] = KF(kfs[k]); vv[k] = MPs(matches + (size_t)k * N1, N1); s[k] = s12s[k];
            R.push_back(Floats(R12s + 9 * k, 3, 3)); t.push_back(Floats(t12s + 3 * k, 3, 1));
        }
        std::vector<int> n;
        if (batch) n = m.SearchBySim3Batch(KF(kf1), v2, vv, s, R, t, th);
        else for (int k = 0; k < K; ++k) n.push_back(m.SearchBySim3(KF(kf1), v2[k], vv[k], s[k], R[k], t[k], th));
        if ((int)n.size() != K) throw std::runtime_error("wrong number of results");
        for (int k = 0; k < K; ++k) { counts[k] = n[k]; Put(vv[k], matches + (size_t)k * N1); }
    });
}
}
