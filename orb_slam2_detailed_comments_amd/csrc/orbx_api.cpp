// orbx_api.cpp -- the core of the C ABI of liborbx.so (include/orbx.h): the error record, names and defaults, the handle's
// lifecycle (orbx_create / configure / orbx_destroy), the getters, the staging every other unit shares (orbx_handle.h), and the
// stream / timing / profile calls.  The subsystems' entry points live in one unit each: orbx_extract.cpp, orbx_pyramid.cpp,
// orbx_match.cpp, orbx_tracking.cpp, orbx_map_batches.cpp, orbx_bow.cpp, orbx_policies.cpp, orbx_kfdb.cpp.
#include <dlfcn.h>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include "orbx_handle.h"

static thread_local std::string g_last_error;
orbx_status orbx_fail(orbx_status s, const std::string &msg) {
    g_last_error = msg;
    return s;
}

static const char *k_names[ORBX_K_COUNT] = {"k_pyr_l0", "k_pyr_resize", "k_fast_rows", "k_quadtree", "k_orient",
                                            "k_blur",   "k_describe",   "k_match",      "misc"};

extern "C" const char *orbx_kernel_name(int k) { return (k >= 0 && k < ORBX_K_COUNT) ? k_names[k] : "?"; }
extern "C" const char *orbx_last_error(void) { return g_last_error.c_str(); }
extern "C" int orbx_abi_version(void) { return ORBX_ABI_VERSION; }
extern "C" const char *orbx_status_string(orbx_status s) {
    switch (s) {
        case ORBX_OK: return "ok";
        case ORBX_EMPTY_IMAGE: return "empty image";
        case ORBX_BAD_ARGUMENT: return "bad argument";
        case ORBX_BAD_ASPECT: return "bad aspect ratio (nIni == 0)";
        case ORBX_CAPACITY: return "capacity exceeded";
        case ORBX_HIP_ERROR: return "HIP error";
        case ORBX_NO_DEVICE: return "no HIP device";
        case ORBX_UNSUPPORTED: return "unsupported geometry";
    }
    return "?";
}

extern "C" void orbx_default_params(orbx_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->nfeatures = 1000; p->scale_factor = 1.2f; p->nlevels = 8; p->ini_th_fast = 20; p->min_th_fast = 7;
    p->pyramid_mode = ORBX_PYRAMID_FORK_PADDED; p->fp_mode = ORBX_FP_GCC_FMA;
    p->device = -1; p->max_batch = 1; p->max_cand_per_cell = 0;
}

// ---------------------------------------------------------------- profiling helpers
// roctx ranges around every stage's launches: ORBX_ROCTX=1 loads the roctx library at the first use and
// brackets each ProfScope with roctxRangePushA(slot name) / roctxRangePop, so `rocprofv3 --marker-trace` groups the
// kernels of a call by stage.  Not linked: without the variable the library has no dependency on the profiler.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char *e = getenv("ORBX_ROCTX");
        if (!e || !atoi(e)) return;
        void *lib = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);   // the one rocprofv3 --marker-trace records
        if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);                 // roctracer's (older tools)
        if (!lib) return;
        push = (int (*)(const char *))dlsym(lib, "roctxRangePushA");
        pop = (int (*)())dlsym(lib, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
static const Roctx &roctx() { static Roctx r; return r; }
// ProfScope (orbx_handle.h) reaches the two entry points through these
bool orbx_roctx_push(const char *name) { if (!roctx().push) return false; roctx().push(name); return true; }
void orbx_roctx_pop() { roctx().pop(); }

void prof_drain(orbx_handle *h) {
    if (h->pending.empty()) return;
    hipStreamSynchronize(h->stream);
    for (auto &pp : h->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pp.a, pp.b) == hipSuccess) { h->ms[pp.kid] += ms; h->launches[pp.kid]++; }
        h->pool.push_back(pp.a); h->pool.push_back(pp.b);
    }
    h->pending.clear();
}

// ---------------------------------------------------------------- workspace
static void free_geometry_buffers(orbx_handle *h) {
    hipFree(h->d_groups); h->d_groups = nullptr;
    hipFree(h->d_pyr); hipFree(h->d_blur); hipFree(h->d_cells); hipFree(h->d_taps);
    hipFree(h->d_dense); h->d_dense = nullptr;
    hipFree(h->d_cand_count); hipFree(h->d_lvl_count); hipFree(h->d_status); hipFree(h->d_lvl_kp);
    hipFree(h->d_lvl_angle); hipFree(h->d_knode);
    hipFree(h->d_l0_scratch); h->d_l0_scratch = nullptr; h->l0_pending = false;
    h->d_pyr = h->d_blur = nullptr; h->d_cells = nullptr; h->d_taps = nullptr;
    h->d_cand_count = h->d_lvl_count = h->d_status = nullptr; h->d_lvl_kp = nullptr; h->d_lvl_angle = nullptr;
    h->d_knode = nullptr;
    h->configured = false;
}

orbx_status read_fast_gpw(orbx_handle *h) {
    h->fast_gpw = 0;
    if (const char *e = getenv("ORBX_FAST_GPW")) {   // tests run two planted groups per wave at a batch of 16 frames with it
        if (strcmp(e, "1") == 0 || strcmp(e, "2") == 0) h->fast_gpw = e[0] - '0';
        else return orbx_fail(ORBX_BAD_ARGUMENT, "ORBX_FAST_GPW must be 1 or 2");
    }
    return ORBX_OK;
}

orbx_status configure(orbx_handle *h, int width, int height) {
    if (h->configured && h->geom.width == width && h->geom.height == height) return ORBX_OK;
    if (h->host_only) return orbx_fail(ORBX_NO_DEVICE, "host-only handle (device = -2) cannot extract");
    HIPCHK(hipSetDevice(h->dev));
    if (h->configured) {   // nothing queued on any of the handle's streams may still read the buffers that are about to go
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->side_stream) HIPCHK(hipStreamSynchronize(h->side_stream));
        if (h->plan_stream) HIPCHK(hipStreamSynchronize(h->plan_stream));
        free_geometry_buffers(h);
    }
    const char *why = "";
    OrbxGeom g;
    orbx_status st = orbx_build_geometry(h->p, h->tab, width, height, g, &why);
    if (st != ORBX_OK) return orbx_fail(st, why);
    h->geom = g;
    const int B = h->p.max_batch, NL = h->p.nlevels;
    // device geometry block
    DGeom &d = h->dg;
    memset(&d, 0, sizeof(d));
    d.nlevels = NL; d.ncells = (int)g.cells.size(); d.kp_total = g.kp_total; d.fp_mode = h->p.fp_mode;
    d.ini_th = std::min(std::max(h->p.ini_th_fast, 0), 255);
    d.min_th = std::min(std::max(h->p.min_th_fast, 0), 255);
    d.pyr_bytes = g.pyr_bytes; d.cand_total = g.cand_total;
    for (int i = 0; i < 16; ++i) d.umax[i] = h->tab.umax[i];
    int tiles = 0;
    h->max_cw = h->max_ch = 7;
    for (const auto &c : g.cells) { h->max_cw = std::max<int>(h->max_cw, c.cw); h->max_ch = std::max<int>(h->max_ch, c.ch); }
    for (int l = 0; l < NL; ++l) {
        const OrbxLevelGeom &L = g.lv[l];
        DLevel &D = d.lv[l];
        D.pw = L.pw; D.ph = L.ph; D.pitch = L.pitch; D.sw = L.sw; D.sh = L.sh;
        D.cell_begin = L.cell_begin; D.cell_count = L.cell_count;
        D.qt_w = L.qt_w; D.qt_h = L.qt_h; D.nini = L.nini; D.hx = L.hx;
        D.nfeat = L.nfeat; D.kp_cap = L.kp_cap; D.kp_begin = L.kp_begin; D.cand_cap = L.cand_cap;
        D.tapx = L.tapx_begin; D.tapy = L.tapy_begin; D.scale = L.scale; D.size = L.size;
        D.off = L.off; D.cand_begin = L.cand_begin; D.org = L.org;
        D.blur_tx = (L.pw + 127) / 128;  // k_blur tile = 128 x 32
        D.blur_tile_begin = tiles;
        tiles += D.blur_tx * ((L.ph + 31) / 32);
    }
    d.blur_tiles = tiles;
    // quadtree LDS plan: node tables always in LDS; keys in registers when the level's candidates fit them (qt_reg_keys below),
    // else key->node map in LDS when they fit the key slots
    h->ncap = g.node_cap;
    // Keys of a level (position + node index, 6 bytes each) live in LDS when they fit `lds_keys` slots; denser levels fall
    // back to the global scratch map (same code path through a generic pointer).  The kernel is latency-bound (a chain of
    // barrier-separated stages), so what counts is how many workgroups a CU holds: take the largest residency (4 = the wave
    // limit of 512-thread workgroups, then 3, 2, 1) whose key slots still cover ~6 candidates per kept keypoint of the
    // densest level (level 0 of the 640x480 bench frames has 1230 candidates for 217 keypoints), capped at 4096.
    const size_t node_part = orbx_quadtree_smem(h->ncap, 0);
    if (node_part > 120 * 1024) return orbx_fail(ORBX_UNSUPPORTED, "nfeatures too large for the LDS quadtree node table");
    {
        const size_t want = std::min<size_t>({(size_t)4096, (size_t)g.max_cand_cap, (size_t)6 * (size_t)std::max(g.lv[0].nfeat, 1)});
        size_t keys = 0;
        auto fit_at = [&](int wg) -> size_t {
            const size_t budget = (size_t)(160 * 1024) / wg - 512;   // allocation granularity margin
            return budget <= node_part ? 0 : std::min<size_t>({(budget - node_part) / 6, (size_t)4096, (size_t)g.max_cand_cap});
        };
        // ... and no more than that: key slots beyond `want` only lower the number of workgroups a CU can hold (1024-frame
        // batches, 640x480 / 1000 features: 2794 slots = 4 workgroups per CU 250 us, 1400 slots 204 us, 600 slots 208 us).
        // (Launching the small levels on their own with a node table and key slots sized for them -- more workgroups per CU
        // still -- measured 215-220 us against 200, and 277 against 259 us at 1920x1080 / 4000 features where the common plan
        // admits one workgroup per CU: the large levels set the time, and the second launch boundary is pure cost.)
        // Small launches (a few workgroups per CU at most: the single-frame call) have nothing to gain from residency and take
        // the plan that fills the budget, so that the densest level keeps its keys in LDS too (lds_keys_few).
        size_t keys_few = 0;
        for (int wg = 4; wg >= 2 && keys == 0; --wg)
            if (fit_at(wg) >= want) { keys = std::max<size_t>(want, 1024); keys_few = fit_at(wg); }
        h->lds_keys_few = (int)keys_few;
        // large nfeatures (node tables of tens of KB): two workgroups per CU with the dense levels on the global key map beat
        // one workgroup with every level in LDS -- those levels exceed any LDS budget anyway
        if (keys == 0 && fit_at(2) >= 1024) keys = fit_at(2);
        if (keys == 0) keys = fit_at(1);
        // Register-resident keys (k_quadtree): a workgroup of T threads keeps up to qt_reg_keys * T keys in registers and needs
        // no key slots at all.  ORBX_QT_REG_KEYS = 0..ORBX_QT_KPT moves that boundary (tests, A/B runs); 0 is the LDS / global
        // plan alone.  Where the registers of the smallest workgroup (256 threads) cover what the residency plan sized its
        // slots for, the plan drops them: the node tables alone admit 8 workgroups of 256 threads per CU at 1000 features
        // instead of 6, and a workgroup that overflows the registers takes the global key map.
        h->qt_reg_keys = ORBX_QT_KPT;
        if (const char *e = getenv("ORBX_QT_REG_KEYS")) h->qt_reg_keys = std::min(std::max(atoi(e), 0), ORBX_QT_KPT);
        if ((size_t)h->qt_reg_keys * 256 >= want) keys = 0;
        if (const char *e = getenv("ORBX_QT_LDS_KEYS")) keys = std::min<size_t>((size_t)std::max(atoi(e), 0), std::min<size_t>(8192, (160 * 1024 - node_part) / 6));
        h->lds_keys = (int)keys;
        if (getenv("ORBX_QT_LDS_KEYS") || h->lds_keys_few < h->lds_keys) h->lds_keys_few = h->lds_keys;
    }
    HIPCHK(orbx_quadtree_prepare(orbx_quadtree_smem(h->ncap, std::max(h->lds_keys, h->lds_keys_few))));
    // buffers.  Every fill / upload below is issued on the handle's stream: the kernels that read them are launched on
    // the same stream, so the order holds by construction (hipMemset on the NULL stream is asynchronous and NOT ordered
    // with a non-blocking stream -- the round-1 race -- and a device-wide barrier would stall every other handle).
    // Source vectors live in h->geom (they outlive the copies).
    if (const char *e = getenv("ORBX_RESIZE_IMPL")) h->resize_legacy = strcmp(e, "legacy") == 0;
    h->rr_rpw = 0;
    if (const char *e = getenv("ORBX_RR_RPW")) {   // tests reach every trip shape of the row walk at tiny batches with it; sweeps
        const int v = atoi(e);
        if (v >= 2 && v <= 64 && (v & (v - 1)) == 0) h->rr_rpw = v;
        else return orbx_fail(ORBX_BAD_ARGUMENT, "ORBX_RR_RPW must be a power of two in 2..64");
    }
#ifdef ORBX_TIMING_KNOBS   // phase-timing builds only (tools/build_variant.sh): stops k_fast_rows early, results are wrong
    if (const char *e = getenv("ORBX_FAST_STOP")) h->fast_stop = atoi(e);
#endif
    if (const char *e = getenv("ORBX_FAST_LCAP")) h->fast_lcap = std::max(64, atoi(e));
    { const orbx_status gs = read_fast_gpw(h);
      if (gs != ORBX_OK) return gs; }
    const OrbxGeom &hg = h->geom;
    hipStream_t s = h->stream;
    // Optional fork of the batched launch sequence (run_chunk): ORBX_FORK_LEVEL = l > 0 resizes levels >= l and runs their
    // FAST groups on the side stream next to the FAST kernel of the large levels (+1..3 % frames/s at l = 3 or 4 for 256-frame
    // batches).  Off by default: the gain is small and kernels that share the chip have durations that no longer describe
    // the kernel alone.
    h->fork_level = 0;
    if (const char *e = getenv("ORBX_FORK_LEVEL")) h->fork_level = std::min(std::max(atoi(e), 0), NL - 1);
    h->fork_group = 0;
    if (h->fork_level > 0) {
        while (h->fork_group < (int)hg.fast_groups.size() && hg.cells[(size_t)hg.fast_groups[(size_t)h->fork_group].cell0].level < h->fork_level)
            ++h->fork_group;
        if (h->fork_group == 0 || h->fork_group >= (int)hg.fast_groups.size()) h->fork_level = 0;
    }
    // The sub-batch pipeline (run_chunk) and the fork exclude each other, both use the side stream: an explicit
    // ORBX_FORK_LEVEL > 0 (an A/B knob) selects the fork and the serial sub-batch sequence.
    h->pipeline = 2;
    if (const char *e = getenv("ORBX_PIPELINE")) h->pipeline = std::min(std::max(atoi(e), 0), ORBX_PIPE_MAX);
    h->l0_inplace = true;
    if (const char *e = getenv("ORBX_LEVEL0_INPLACE")) h->l0_inplace = atoi(e) != 0;
    h->l0_eager_sticky = false;   // a new geometry starts over
    if (const char *e = getenv("ORBX_PIPELINE_HEAD")) h->pipe_head = atoi(e) != 0;
    if (const char *e = getenv("ORBX_FAST_ROOM")) h->fast_room = atoi(e) != 0;
    h->fast_first = true;
    if (getenv("ORBX_PIPELINE")) {
        h->fast_first = false;
    } else if (const char *e = getenv("ORBX_PLAN")) {   // "pipeline": the sub-batch pipeline with its own defaults
        h->fast_first = strcmp(e, "fastfirst") == 0;
        if (strcmp(e, "serial") == 0) h->pipeline = 0;
    }
    if (const char *e = getenv("ORBX_PLAN_SUB")) h->plan_sub = std::min(std::max(atoi(e), 1), ORBX_PIPE_MAX);
    if (const char *e = getenv("ORBX_PLAN_HEAD")) h->plan_head = atoi(e) != 0;
    h->plan_min_frames = ORBX_PIPE_MIN_FRAMES;
    if (const char *e = getenv("ORBX_PLAN_MIN_FRAMES")) h->plan_min_frames = std::max(atoi(e), 1);
    if (h->fork_level > 0) { h->pipeline = 0; h->fast_first = false; }
    h->l0_groups = 0;
    h->max_ch_l0 = h->max_ch_rest = 7;
    for (const OrbxFastGroup &fg : hg.fast_groups) {
        const bool l0 = hg.cells[(size_t)fg.cell0].level == 0;
        if (l0) ++h->l0_groups;
        for (int c = 0; c < fg.ncell; ++c) {
            int &m = l0 ? h->max_ch_l0 : h->max_ch_rest;
            m = std::max<int>(m, hg.cells[(size_t)fg.cell0 + c].ch);
        }
    }
    auto setup = [&]() -> hipError_t {
        hipError_t e;
#define ORBX_TRY(expr) do { e = (expr); if (e != hipSuccess) return e; } while (0)
        ORBX_TRY(hipMalloc(&h->d_pyr, (size_t)B * hg.pyr_bytes + 256));   // +256: kernels read whole aligned dwords
        ORBX_TRY(hipMalloc(&h->d_cells, std::max<size_t>(1, hg.cells.size()) * sizeof(OrbxCell)));
        ORBX_TRY(hipMalloc(&h->d_taps, std::max<size_t>(1, hg.taps.size()) * sizeof(OrbxTap)));
        ORBX_TRY(hipMalloc(&h->d_dense, (size_t)B * hg.cand_total * sizeof(uint2)));
        ORBX_TRY(hipMalloc(&h->d_knode, (size_t)B * hg.cand_total * sizeof(uint16_t)));
        ORBX_TRY(hipMalloc(&h->d_cand_count, (size_t)B * NL * sizeof(int)));
        ORBX_TRY(hipMalloc(&h->d_lvl_count, (size_t)B * NL * sizeof(int)));
        ORBX_TRY(hipMalloc(&h->d_status, (size_t)B * sizeof(int)));
        ORBX_TRY(hipMalloc(&h->d_l0_scratch, (size_t)B * (NL + 1) * sizeof(int)));
        ORBX_TRY(hipMalloc(&h->d_lvl_kp, (size_t)B * hg.kp_total * sizeof(uint32_t)));
        ORBX_TRY(hipMalloc(&h->d_lvl_angle, (size_t)B * hg.kp_total * sizeof(float)));
        ORBX_TRY(hipMalloc(&h->d_groups, std::max<size_t>(1, hg.fast_groups.size()) * sizeof(OrbxFastGroup)));
        if (!hg.cells.empty()) {
            ORBX_TRY(hipMemcpyAsync(h->d_cells, hg.cells.data(), hg.cells.size() * sizeof(OrbxCell), hipMemcpyHostToDevice, s));
            ORBX_TRY(hipMemcpyAsync(h->d_groups, hg.fast_groups.data(), hg.fast_groups.size() * sizeof(OrbxFastGroup),
                                    hipMemcpyHostToDevice, s));
        }
        if (!hg.taps.empty())
            ORBX_TRY(hipMemcpyAsync(h->d_taps, hg.taps.data(), hg.taps.size() * sizeof(OrbxTap), hipMemcpyHostToDevice, s));
        ORBX_TRY(hipMemsetAsync(h->d_pyr, 0, (size_t)B * hg.pyr_bytes + 256, s));
        ORBX_TRY(hipMemsetAsync(h->d_lvl_count, 0, (size_t)B * NL * sizeof(int), s));
        ORBX_TRY(hipMemsetAsync(h->d_cand_count, 0, (size_t)B * NL * sizeof(int), s));
#undef ORBX_TRY
        return hipSuccess;
    };
    const hipError_t se = setup();
    if (se != hipSuccess) {   // nothing half-allocated survives a failed configure()
        hipStreamSynchronize(s);
        free_geometry_buffers(h);
        return orbx_fail(ORBX_HIP_ERROR, std::string("configure: ") + hipGetErrorString(se));
    }
    h->configured = true;
    h->last_batch = 0;
    return ORBX_OK;
}

extern "C" orbx_status orbx_create(const orbx_params *params, orbx_handle **out) {
    if (!params || !out) return orbx_fail(ORBX_BAD_ARGUMENT, "null argument");
    *out = nullptr;
    if (params->nlevels < 1 || params->nlevels > ORBX_MAX_LEVELS) return orbx_fail(ORBX_BAD_ARGUMENT, "nlevels out of range [1,16]");
    if (params->nfeatures < 1 || params->nfeatures > 16000) return orbx_fail(ORBX_BAD_ARGUMENT, "nfeatures out of range [1,16000]");
    if (!(params->scale_factor > 1.0f)) return orbx_fail(ORBX_BAD_ARGUMENT, "scale_factor must be > 1");
    if (params->pyramid_mode != ORBX_PYRAMID_FORK_PADDED && params->pyramid_mode != ORBX_PYRAMID_UPSTREAM)
        return orbx_fail(ORBX_UNSUPPORTED, "pyramid_mode: ORBX_PYRAMID_FORK_PADDED and ORBX_PYRAMID_UPSTREAM are implemented");
    if (params->fp_mode != ORBX_FP_GCC_FMA && params->fp_mode != ORBX_FP_STRICT) return orbx_fail(ORBX_BAD_ARGUMENT, "fp_mode");
    orbx_handle *h = new orbx_handle();
    h->p = *params;
    if (h->p.max_batch < 1) h->p.max_batch = 1;
    if (const char *e = getenv("ORBX_MATCH_KERNEL")) h->match_kernel = strcmp(e, "valu") == 0 ? 1 : strcmp(e, "i8") == 0 ? 2 : 0;
    orbx_build_tables(h->p, h->tab);
    static_assert(ORBX_PS_LEVELS >= ORBX_MAX_LEVELS, "one threshold per level");
    orbx_predict_scale_build(orbx_get_scale_factor(h), h->p.nlevels, h->ps_thr);
    if (params->device == -2) {  // host-only handle: tables and getters, no device work
        h->host_only = true;
        *out = h;
        return ORBX_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        delete h;
        return orbx_fail(ORBX_NO_DEVICE, "no HIP device visible: the ORB front-end has no CPU fallback");
    }
    int dev = params->device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= ndev) { delete h; return orbx_fail(ORBX_BAD_ARGUMENT, "device ordinal out of range"); }
    h->dev = dev;
    hipError_t e = hipSetDevice(dev);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = orbx_upload_pattern();
    if (e == hipSuccess) {
        int lo = 0, hi = 0;
        e = hipDeviceGetStreamPriorityRange(&lo, &hi);   // hi = numerically lowest = highest priority
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&h->side_stream, hipStreamNonBlocking, hi);
        // the FAST-first plan's resize chains: LOW priority by default (lo = numerically highest), ORBX_PLAN_PRIORITY=low|normal|high
        // for A/B runs.  FAST is bound by the waves a CU holds; at high priority the resize waves take their slots first and
        // FAST stretches by nearly the time the chains take, at low priority they fill what FAST leaves (profiles/fast_first_plan.md)
        int prio = lo;
        if (const char *pe = getenv("ORBX_PLAN_PRIORITY")) prio = strcmp(pe, "high") == 0 ? hi : strcmp(pe, "normal") == 0 ? 0 : lo;
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&h->plan_stream, hipStreamNonBlocking, prio);
        // device-scope release: the two streams exchange device memory only (a system-scope fence per record costs ~10 us)
        unsigned evflags = hipEventDisableTiming | hipEventReleaseToDevice;
        if (const char *ef = getenv("ORBX_EVENT_FLAGS")) evflags = (unsigned)strtoul(ef, nullptr, 0);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, evflags);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, evflags);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_stereo, evflags);
        for (int k = 0; k < ORBX_PIPE_MAX && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&h->ev_pipe[k], evflags);
    }
    if (e != hipSuccess) { orbx_destroy(h); return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e)); }
    h->stream = h->own_stream;
    *out = h;
    return ORBX_OK;
}

extern "C" void orbx_destroy(orbx_handle *h) {
    if (!h) return;
    if (!h->host_only) {
        hipSetDevice(h->dev);
        hipStreamSynchronize(h->stream);
        prof_drain(h);
        for (auto e : h->pool) hipEventDestroy(e);
        free_geometry_buffers(h);
        hipFree(h->d_match_ws); hipFree(h->d_scratch); hipFree(h->d_rect); hipFree(h->d_gate_items);
        if (h->pin) hipHostFree(h->pin);
        if (h->pin_early) hipHostFree(h->pin_early);
        if (h->ev_stage) hipEventDestroy(h->ev_stage);
        if (h->pin_stat) hipHostFree(h->pin_stat);
        for (int s = 0; s < 2; ++s) {
            hipFree(h->st_in[s]); hipFree(h->st_kps[s]);   // st_desc / st_cnt live inside the st_kps allocation
            hipFree(h->st_dep[s]); hipFree(h->st_rg[s]);
            if (h->ev_in[s]) hipEventDestroy(h->ev_in[s]);
            if (h->ev_done[s]) hipEventDestroy(h->ev_done[s]);
            if (h->ev_out[s]) hipEventDestroy(h->ev_out[s]);
        }
        if (h->s_in) hipStreamDestroy(h->s_in);
        if (h->side_stream) { hipStreamSynchronize(h->side_stream); hipStreamDestroy(h->side_stream); }
        if (h->plan_stream) { hipStreamSynchronize(h->plan_stream); hipStreamDestroy(h->plan_stream); }
        if (h->ev_fork) hipEventDestroy(h->ev_fork);
        if (h->ev_join) hipEventDestroy(h->ev_join);
        if (h->ev_stereo) hipEventDestroy(h->ev_stereo);
        for (auto ev : h->ev_pipe) if (ev) hipEventDestroy(ev);
        if (h->own_stream) hipStreamDestroy(h->own_stream);
    }
    delete h;
}

// ---------------------------------------------------------------- getters
extern "C" int orbx_get_levels(const orbx_handle *h) { return h ? h->p.nlevels : 0; }
extern "C" float orbx_get_scale_factor(const orbx_handle *h) { return h ? (float)(double)h->p.scale_factor : 0.f; }
extern "C" orbx_status orbx_get_scale_tables(const orbx_handle *h, float *scale, float *inv_scale, float *sigma2,
                                             float *inv_sigma2) {
    if (!h) return orbx_fail(ORBX_BAD_ARGUMENT, "null handle");
    const int n = h->p.nlevels;
    if (scale) memcpy(scale, h->tab.scale, n * sizeof(float));
    if (inv_scale) memcpy(inv_scale, h->tab.inv_scale, n * sizeof(float));
    if (sigma2) memcpy(sigma2, h->tab.sigma2, n * sizeof(float));
    if (inv_sigma2) memcpy(inv_sigma2, h->tab.inv_sigma2, n * sizeof(float));
    return ORBX_OK;
}
extern "C" orbx_status orbx_get_features_per_level(const orbx_handle *h, int32_t *n) {
    if (!h || !n) return orbx_fail(ORBX_BAD_ARGUMENT, "null argument");
    memcpy(n, h->tab.nfeat, h->p.nlevels * sizeof(int32_t));
    return ORBX_OK;
}
extern "C" orbx_status orbx_get_umax(const orbx_handle *h, int32_t *umax16) {
    if (!h || !umax16) return orbx_fail(ORBX_BAD_ARGUMENT, "null argument");
    memcpy(umax16, h->tab.umax, 16 * sizeof(int32_t));
    return ORBX_OK;
}
extern "C" int orbx_max_keypoints(orbx_handle *h, int width, int height) {
    if (!h || width <= 0 || height <= 0) return -(int)ORBX_BAD_ARGUMENT;
    if (h->configured && h->geom.width == width && h->geom.height == height) return h->geom.kp_total;
    if (h->mk_w == width && h->mk_h == height) return h->mk_total;
    OrbxGeom g; const char *why = "";
    const orbx_status st = orbx_build_geometry(h->p, h->tab, width, height, g, &why);
    if (st != ORBX_OK) { g_last_error = why; return -(int)st; }
    h->mk_w = width; h->mk_h = height; h->mk_total = g.kp_total;
    return g.kp_total;
}

// ---------------------------------------------------------------- staging (orbx_handle.h): device arena + page-locked block
orbx_status dev_grow(orbx_handle *h, void **p, size_t *cap, size_t need, size_t want, size_t elem) {
    if (need <= *cap) return ORBX_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    hipFree(*p); *p = nullptr; *cap = 0;
    HIPCHK(hipMalloc(p, want * elem));
    *cap = want;
    return ORBX_OK;
}
orbx_status scratch_reserve(orbx_handle *h, size_t bytes) {
    h->scratch_used = 0;
    return dev_grow(h, (void **)&h->d_scratch, &h->scratch_bytes, bytes, std::max(bytes, (size_t)1 << 20));
}
static orbx_status pin_grow(orbx_handle *h, uint8_t **p, size_t *cap, size_t bytes) {   // the one growth rule of both blocks
    if (bytes <= *cap) return ORBX_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (*p) hipHostFree(*p);
    *p = nullptr; *cap = 0;
    const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 20);
    HIPCHK(hipHostMalloc((void **)p, want, hipHostMallocDefault));
    *cap = want;
    return ORBX_OK;
}
orbx_status stage_pin(orbx_handle *h, size_t bytes) { return pin_grow(h, &h->pin, &h->pin_bytes, bytes); }
// (a call that returns early leaves h->pin_early pending: the next one waits for that copy here; steady state does not meet it)
orbx_status stage_begin(orbx_handle *h, size_t pin_bytes, size_t dev_bytes, uint8_t **pin, uint8_t **dev, bool returns_early) {
    HIPCHK(hipSetDevice(h->dev));
    h->stage_early = returns_early;
    if (returns_early && h->stage_pending) { HIPCHK(hipEventSynchronize(h->ev_stage)); h->stage_pending = false; }
    orbx_status st = returns_early ? pin_grow(h, &h->pin_early, &h->pin_early_bytes, pin_bytes) : stage_pin(h, pin_bytes);
    if (st == ORBX_OK) st = scratch_reserve(h, dev_bytes + 256);
    if (st != ORBX_OK) return st;
    *pin = returns_early ? h->pin_early : h->pin;
    *dev = scratch_take<uint8_t>(h, dev_bytes);
    return ORBX_OK;
}
orbx_status stage_upload(orbx_handle *h, const uint8_t *pin, uint8_t *dev, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, h->stream));
    if (!h->stage_early) return ORBX_OK;
    if (!h->ev_stage) HIPCHK(hipEventCreateWithFlags(&h->ev_stage, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->ev_stage, h->stream));
    h->stage_pending = true;
    return ORBX_OK;
}
orbx_status stage_download_wait(orbx_handle *h, uint8_t *pin, const uint8_t *d_out, size_t bytes) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(pin, d_out, bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return orbx_fail(ORBX_HIP_ERROR, hipGetErrorString(e));
    return ORBX_OK;
}

// ---------------------------------------------------------------- stream / timing
extern "C" void *orbx_get_stream(orbx_handle *h) { return h ? (void *)h->stream : nullptr; }
extern "C" orbx_status orbx_set_stream(orbx_handle *h, void *s) {
    if (!h || h->host_only) return orbx_fail(ORBX_BAD_ARGUMENT, "no device handle");
    hipSetDevice(h->dev);
    hipStreamSynchronize(h->stream);
    prof_drain(h);
    h->stream = s ? (hipStream_t)s : h->own_stream;
    return ORBX_OK;
}
extern "C" orbx_status orbx_synchronize(orbx_handle *h) {
    if (!h || h->host_only) return orbx_fail(ORBX_BAD_ARGUMENT, "no device handle");
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ORBX_OK;
}
extern "C" orbx_status orbx_profile_enable(orbx_handle *h, uint32_t mask) {
    if (!h || h->host_only) return orbx_fail(ORBX_BAD_ARGUMENT, "no device handle");
    prof_drain(h);
    h->prof_mask = mask;
    return ORBX_OK;
}
extern "C" orbx_status orbx_profile_read(orbx_handle *h, float *ms, int32_t *launches, int reset) {
    if (!h || h->host_only) return orbx_fail(ORBX_BAD_ARGUMENT, "no device handle");
    hipSetDevice(h->dev);
    prof_drain(h);
    if (ms) memcpy(ms, h->ms, sizeof(h->ms));
    if (launches) memcpy(launches, h->launches, sizeof(h->launches));
    if (reset) { memset(h->ms, 0, sizeof(h->ms)); memset(h->launches, 0, sizeof(h->launches)); }
    return ORBX_OK;
}
