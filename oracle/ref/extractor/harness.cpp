// oracle/ref/extractor: C ABI over the reference's src/ORBextractor.cc, compiled unmodified.  The source is included by path
// from the reference's include root (the build passes -I<reference>), so that its file-static functions IC_Angle,
// computeOrientation, computeOrbDescriptor and computeDescriptors are callable here; the protected members are reached through
// a derived class.  <opencv2/...> and <opencv/cv.h> resolve to the stand-ins of this directory: see opencv2/core/core.hpp.
//
// F3 made literal: std::sort over pair<int, ExtractorNode*> breaks equal sizes by node ADDRESS.  Unless REF_PLAIN_MALLOC is
// defined, the std::list<ExtractorNode> nodes of this library come from a monotonic arena, so that address order is allocation
// order.  The replaced operator new / delete are kept local by the version script exports.map: they bind inside this library and are not
// exported, so the process that loads the library keeps its own.  Only requests of exactly the list node's size are served
// from the arena (nothing else in the reference is compared by address); every other size goes to malloc.  The arena is
// rewound at each entry that runs the quadtree, provided nothing in it is alive.
#include <cstdint>
#include <cstdlib>
#include <new>
#include <src/ORBextractor.cc>

using namespace ORB_SLAM2;

namespace {

#ifndef REF_PLAIN_MALLOC
const size_t NODE_BYTES = sizeof(std::_List_node<ExtractorNode>);
const size_t ARENA_BYTES = (size_t)256 << 20;
char *g_arena = 0;
size_t g_arena_used = 0;
long g_arena_live = 0;       // a rewind with anything alive would hand a live address out again: it waits instead

void arena_rewind() { if (g_arena_live == 0) g_arena_used = 0; }
void *arena_take(size_t n)
{
    if (!g_arena) {
        g_arena = (char *)std::malloc(ARENA_BYTES);   // untouched pages cost nothing
        if (!g_arena) cv::standin_abort("no memory for the list node arena");
    }
    n = (n + 15) & ~(size_t)15;
    if (g_arena_used + n > ARENA_BYTES) cv::standin_abort("list node arena exhausted");
    void *p = g_arena + g_arena_used;
    g_arena_used += n;
    ++g_arena_live;
    return p;
}
bool in_arena(void *p) { return g_arena && (char *)p >= g_arena && (char *)p < g_arena + ARENA_BYTES; }
#else
void arena_rewind() {}
#endif

struct FastCall { int level, x0, y0, w, h, threshold, n; };

struct Ext : ORBextractor {
    std::vector<FastCall> calls;
    std::vector<std::vector<cv::KeyPoint> > cand;       // per level, in call order, relative to (minBorderX, minBorderY)
    std::vector<std::vector<cv::KeyPoint> > levelKeys;  // per level, after ComputeKeyPointsOctTree (with angles)
    Ext(int nf, float sf, int nl, int ini, int mn) : ORBextractor(nf, sf, nl, ini, mn), cand(nl), levelKeys(nl) {}
    void stages(cv::Mat image)
    {
        ComputePyramid(image);
        std::vector<std::vector<cv::KeyPoint> > all;
        ComputeKeyPointsOctTree(all);
        levelKeys = all;
    }
    std::vector<cv::KeyPoint> distribute(const std::vector<cv::KeyPoint> &keys, int minX, int maxX, int minY, int maxY, int N)
    {
        return DistributeOctTree(keys, minX, maxX, minY, maxY, N, 0);
    }
    const std::vector<int> &umaxTable() const { return umax; }
    const std::vector<cv::Point> &patternTable() const { return pattern; }
    const std::vector<int> &quotas() const { return mnFeaturesPerLevel; }
};

Ext *g_recording = 0;

void record_fast(const cv::Mat &image, int threshold, const std::vector<cv::KeyPoint> &keys)
{
    Ext *e = g_recording;
    if (!e) return;
    int level = -1;
    for (int l = 0; l < e->GetLevels(); ++l)
        if (image.shares(e->mvImagePyramid[l])) { level = l; break; }
    if (level < 0) cv::standin_abort("FAST on an image that is no pyramid level");
    const cv::Mat &pyr = e->mvImagePyramid[level];
    size_t off = (size_t)(image.data - pyr.data);
    FastCall c = {level, (int)(off % (size_t)pyr.step), (int)(off / (size_t)pyr.step), image.cols, image.rows, threshold, (int)keys.size()};
    e->calls.push_back(c);
    for (size_t i = 0; i < keys.size(); ++i) {
        cv::KeyPoint k = keys[i];
        k.pt.x += (float)(c.x0 - (EDGE_THRESHOLD - 3));
        k.pt.y += (float)(c.y0 - (EDGE_THRESHOLD - 3));
        e->cand[level].push_back(k);
    }
}

Ext &shared()
{
    static Ext *e = new Ext(1000, 1.2f, 8, 20, 7);
    return *e;
}

}  // namespace

#ifndef REF_PLAIN_MALLOC
#define HIDDEN   /* exports.map makes them local: <new> declares them with default visibility, so an attribute here is ignored */
HIDDEN void *operator new(size_t n)
{
    void *p = n == NODE_BYTES ? arena_take(n) : std::malloc(n ? n : 1);
    if (!p) throw std::bad_alloc();
    return p;
}
HIDDEN void *operator new[](size_t n) { return operator new(n); }
HIDDEN void operator delete(void *p) noexcept
{
    if (!p) return;
    if (in_arena(p)) --g_arena_live;
    else std::free(p);
}
HIDDEN void operator delete[](void *p) noexcept { operator delete(p); }
HIDDEN void operator delete(void *p, size_t) noexcept { operator delete(p); }
HIDDEN void operator delete[](void *p, size_t) noexcept { operator delete(p); }
#endif

extern "C" {

int h_fp_fast_fma()
{
#ifdef __FMA__
    return 1;
#else
    return 0;
#endif
}

int rx_plain_malloc()
{
#ifdef REF_PLAIN_MALLOC
    return 1;
#else
    return 0;
#endif
}

int rx_list_node_bytes() { return (int)sizeof(std::_List_node<ExtractorNode>); }

void *rx_create(int nfeatures, float scale_factor, int nlevels, int ini_th, int min_th)
{
    return new Ext(nfeatures, scale_factor, nlevels, ini_th, min_th);
}

void rx_destroy(void *h) { delete (Ext *)h; }

void rx_tables(void *h, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2, int *features_per_level, int *umax16)
{
    Ext *e = (Ext *)h;
    std::vector<float> a = e->GetScaleFactors(), b = e->GetInverseScaleFactors(), c = e->GetScaleSigmaSquares(),
                       d = e->GetInverseScaleSigmaSquares();
    for (int i = 0; i < e->GetLevels(); ++i) {
        scale[i] = a[i]; inv_scale[i] = b[i]; sigma2[i] = c[i]; inv_sigma2[i] = d[i];
        features_per_level[i] = e->quotas()[i];
    }
    for (int i = 0; i < 16; ++i) umax16[i] = e->umaxTable()[i];
}

// operator() on the caller's image; keypoints and descriptors in the reference's order.  Returns the count; -1 when
// operator() returned without touching its outputs (empty image); -4 when cap is too small.  A second pass then runs
// ComputePyramid and ComputeKeyPointsOctTree on their own, for rx_level_keypoints.
int rx_extract(void *h, const uint8_t *img, int w, int hgt, int stride, orc_keypoint *kps, uint8_t *desc, int cap)
{
    Ext *e = (Ext *)h;
    arena_rewind();
    e->calls.clear();
    for (size_t l = 0; l < e->cand.size(); ++l) { e->cand[l].clear(); e->levelKeys[l].clear(); }
    cv::Mat image = (img && w > 0 && hgt > 0) ? cv::Mat(hgt, w, CV_8UC1, (void *)img, (size_t)stride) : cv::Mat();
    std::vector<cv::KeyPoint> keys(1);
    keys[0].class_id = -12345;                      // sentinel: still there after a silent return
    cv::Mat descriptors;
    g_recording = e;
    cv::fast_hook() = record_fast;
    (*e)(image, cv::Mat(), keys, descriptors);
    cv::fast_hook() = 0;
    g_recording = 0;
    if (keys.size() == 1 && keys[0].class_id == -12345) return -1;
    int n = (int)keys.size();
    if (n != descriptors.rows && !(n == 0 && descriptors.empty())) cv::standin_abort("keypoints and descriptor rows differ");
    if (n > cap) return -4;
    if (n) std::memcpy(kps, keys.data(), (size_t)n * sizeof(orc_keypoint));
    for (int i = 0; i < n; ++i) std::memcpy(desc + (size_t)i * 32, descriptors.ptr(i), 32);
    arena_rewind();
    e->stages(image);
    return n;
}

int rx_level_dims(void *h, int level, int *w, int *hgt)
{
    Ext *e = (Ext *)h;
    if (level < 0 || level >= e->GetLevels() || e->mvImagePyramid[level].empty()) return -1;
    *w = e->mvImagePyramid[level].cols; *hgt = e->mvImagePyramid[level].rows;
    return 0;
}

void rx_level_image(void *h, int level, uint8_t *out)   // padded, packed with step = width
{
    const cv::Mat &m = ((Ext *)h)->mvImagePyramid[level];
    for (int y = 0; y < m.rows; ++y) std::memcpy(out + (size_t)y * m.cols, m.ptr(y), (size_t)m.cols);
}

int rx_level_keypoints(void *h, int level, orc_keypoint *out, int cap)
{
    const std::vector<cv::KeyPoint> &k = ((Ext *)h)->levelKeys[level];
    for (int i = 0; i < (int)k.size() && i < cap; ++i) std::memcpy(out + i, &k[i], sizeof(orc_keypoint));
    return (int)k.size();
}

int rx_level_candidates(void *h, int level, orc_keypoint *out, int cap)
{
    const std::vector<cv::KeyPoint> &k = ((Ext *)h)->cand[level];
    for (int i = 0; i < (int)k.size() && i < cap; ++i) std::memcpy(out + i, &k[i], sizeof(orc_keypoint));
    return (int)k.size();
}

// every FAST call of the last rx_extract: (level, x0, y0, w, h, threshold, corners) each
int rx_fast_calls(void *h, int *out7, int cap)
{
    const std::vector<FastCall> &c = ((Ext *)h)->calls;
    for (int i = 0; i < (int)c.size() && i < cap; ++i) std::memcpy(out7 + 7 * i, &c[i], sizeof(FastCall));
    return (int)c.size();
}

float rx_ic_angle(const uint8_t *img, int w, int hgt, int stride, float x, float y)
{
    cv::Mat image(hgt, w, CV_8UC1, (void *)img, (size_t)stride);
    return IC_Angle(image, cv::Point2f(x, y), shared().umaxTable());
}

void rx_descriptor(const uint8_t *img, int w, int hgt, int stride, float x, float y, float angle_deg, uint8_t *desc32)
{
    cv::Mat image(hgt, w, CV_8UC1, (void *)img, (size_t)stride);
    cv::KeyPoint k;
    k.pt.x = x; k.pt.y = y; k.angle = angle_deg;
    computeOrbDescriptor(k, image, &shared().patternTable()[0], desc32);
}

// DistributeOctTree on the caller's key list; out_idx: the selected input indices in the reference's list order
int rx_distribute_octtree(void *h, const orc_keypoint *keys, int nkeys, int minX, int maxX, int minY, int maxY, int N,
                          int *out_idx, int cap)
{
    Ext *e = h ? (Ext *)h : &shared();
    arena_rewind();
    std::vector<cv::KeyPoint> in((size_t)nkeys);
    for (int i = 0; i < nkeys; ++i) {
        std::memcpy(&in[i], keys + i, sizeof(orc_keypoint));
        in[i].class_id = i;
    }
    std::vector<cv::KeyPoint> out = e->distribute(in, minX, maxX, minY, maxY, N);
    for (int i = 0; i < (int)out.size() && i < cap; ++i) out_idx[i] = out[i].class_id;
    return (int)out.size();
}

}  // extern "C"
