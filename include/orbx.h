/* orbx.h -- C ABI of the MI355X-native ORB front-end (liborbx.so).
 *
 * The reference (cheukwaylee/ORB_SLAM2_detailed_comments) has no FFI layer: the boundary of
 * the hot path is the C++ class surface of ORB_SLAM2::ORBextractor (include/ORBextractor.h:82-185)
 * and ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:54-225).  Every entry point below names the
 * reference interface it replaces; compat/ORBextractor.h + compat/ORBmatcher.h are the drop-in
 * C++ classes a maintainer compiles against this ABI.
 *
 * Plain pointers and sizes only; no C++/torch/HIP types in any signature.  "device pointer"
 * arguments are ordinary HIP device addresses (e.g. torch.Tensor.data_ptr()).
 *
 * Threading (mirrors src/Frame.cc:158-168): distinct handles are fully concurrent (one HIP
 * stream + private workspace each); one handle is not re-entrant.
 */
#ifndef ORBX_H
#define ORBX_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_ABI_VERSION 1

/* Bit-compatible with cv::KeyPoint (28 bytes): what ORBextractor::operator() appends to
 * std::vector<cv::KeyPoint>& _keypoints (src/ORBextractor.cc:2016-2082). */
typedef struct orbx_keypoint {
    float x, y;       /* pt.  ORBX_PYRAMID_FORK_PADDED: level-0 *padded-image* coordinates, 19 px off the camera model (fork
                       * semantics).  ORBX_PYRAMID_UPSTREAM: un-padded image coordinates, as in upstream ORB-SLAM2 */
    float size;       /* (float)(int)(31 * scale[octave]) */
    float angle;      /* degrees [0,360) */
    float response;   /* FAST score */
    int32_t octave;
    int32_t class_id; /* always -1 */
} orbx_keypoint;

typedef enum orbx_status {
    ORBX_OK = 0,
    ORBX_EMPTY_IMAGE = 1,   /* reference: silent return, outputs untouched (src/ORBextractor.cc:1966-1967) */
    ORBX_BAD_ARGUMENT = 2,
    ORBX_BAD_ASPECT = 3,    /* nIni == 0: reference divides by zero (src/ORBextractor.cc:1059-1063) */
    ORBX_CAPACITY = 4,      /* caller buffer or internal candidate capacity too small */
    ORBX_HIP_ERROR = 5,
    ORBX_NO_DEVICE = 6,
    ORBX_UNSUPPORTED = 7
} orbx_status;

/* What mvImagePyramid[level] is.  FORK_PADDED: the padded buffer `temp` (the annotated fork's line src/ORBextractor.cc:2166,
 * `mvImagePyramid[level] = temp;`).  UPSTREAM: ComputePyramid without that line, as in upstream ORB-SLAM2 -- the sw x sh view at
 * (19, 19) inside `temp`: level l > 0 is resized from the un-padded level l - 1, the FAST region is [16, sw - 16) x [16, sh - 16),
 * keypoints are in un-padded image coordinates, and SURVEY F6 / F7 do not arise.  A level with sw < 33 or sh < 33 has an empty
 * FAST region there (the reference is undefined): ORBX_UNSUPPORTED, naming the level, before any launch. */
enum { ORBX_PYRAMID_FORK_PADDED = 0, ORBX_PYRAMID_UPSTREAM = 1 };
enum { ORBX_FP_GCC_FMA = 0, ORBX_FP_STRICT = 1 }; /* contraction of GET_VALUE, src/ORBextractor.cc:207-209 */

/* The five values ORBextractor's constructor takes (include/ORBextractor.h:104; read from YAML at
 * src/Tracking.cc:160-168) plus the parity-contract switches and device sizing hints. */
typedef struct orbx_params {
    int32_t nfeatures;
    float scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
    int32_t pyramid_mode;        /* ORBX_PYRAMID_FORK_PADDED (default) or ORBX_PYRAMID_UPSTREAM; per handle */
    int32_t fp_mode;             /* ORBX_FP_GCC_FMA (default parity contract) or ORBX_FP_STRICT */
    int32_t device;              /* HIP device ordinal; -1 = current device */
    int32_t max_batch;           /* frames in flight per call (>=1) */
    int32_t max_cand_per_cell;   /* candidate slots per FAST cell; 0 = exact worst case (never overflows) */
} orbx_params;

typedef struct orbx_handle orbx_handle;

/* ---- lifecycle: replaces `new ORBextractor(nFeatures, fScaleFactor, nLevels, fIniThFAST, fMinThFAST)`
 *      (src/Tracking.cc:171-182) ---------------------------------------------------------- */
orbx_status orbx_create(const orbx_params *params, orbx_handle **out);
void orbx_destroy(orbx_handle *h);
void orbx_default_params(orbx_params *p); /* TUM1.yaml values: 1000, 1.2, 8, 20, 7 */
const char *orbx_last_error(void);        /* thread-local text of the last failure */
const char *orbx_status_string(orbx_status s);
int orbx_abi_version(void);

/* ---- getters: GetLevels / GetScaleFactor(s) / GetInverseScaleFactors / GetScaleSigmaSquares /
 *      GetInverseScaleSigmaSquares (include/ORBextractor.h:120-170), mnFeaturesPerLevel, umax ---- */
int orbx_get_levels(const orbx_handle *h);
float orbx_get_scale_factor(const orbx_handle *h);
orbx_status orbx_get_scale_tables(const orbx_handle *h, float *scale, float *inv_scale,
                                  float *sigma2, float *inv_sigma2); /* nlevels floats each, may be NULL */
orbx_status orbx_get_features_per_level(const orbx_handle *h, int32_t *n_per_level);
orbx_status orbx_get_umax(const orbx_handle *h, int32_t *umax16);
/* output capacity that can never overflow: sum over levels of max(N_l + 3, 4 * nIni_l);
 * < 0: -(orbx_status) (e.g. -ORBX_BAD_ASPECT) */
int orbx_max_keypoints(orbx_handle *h, int width, int height);

/* ---- extraction: replaces ORBextractor::operator()(image, mask, keypoints, descriptors)
 *      (src/ORBextractor.cc:1961-2084; called from Frame::ExtractORB, src/Frame.cc:468-481) ---- */
/* one host frame (8-bit gray, `stride` bytes per row); kps[cap], desc[cap*32]; *n = count */
orbx_status orbx_extract(orbx_handle *h, const uint8_t *img, int width, int height, int stride,
                         orbx_keypoint *kps, uint8_t *desc, int cap, int *n);
/* nframes contiguous host frames (frame_stride bytes apart); outputs [nframes][cap] */
orbx_status orbx_extract_batch(orbx_handle *h, int nframes, const uint8_t *imgs, int width,
                               int height, int stride, int64_t frame_stride, orbx_keypoint *kps,
                               uint8_t *desc, int32_t *counts, int cap);
/* same, all pointers are DEVICE pointers; asynchronous on the handle's stream.  d_status[nframes]
 * receives a per-frame orbx_status (OK / CAPACITY).  No host synchronisation.
 *
 * In-place level 0.  When ALL of these hold the kernels read level 0 IN PLACE from d_imgs and the padded copy of level 0 is
 * not written during the call: this entry point; ORBX_FMT_GRAY8; no rectification maps; d_imgs, `stride` and `frame_stride`
 * multiples of 4; at least 64 x 64 pixels and at least 2 levels; the level-1 tap table passed its footprint check (every usual
 * scale factor); the handle's pyramid_mode is ORBX_PYRAMID_FORK_PADDED (upstream handles always write level 0 during the call);
 * ORBX_RESIZE_IMPL=legacy and ORBX_FORK_LEVEL are not set; the handle's stereo match has not needed the late
 * copy (below); and ORBX_LEVEL0_INPLACE=0 is not set.
 * LIFETIME: in this mode d_imgs is read until the LAST kernel of the call has finished on the handle's stream, not only by
 * its first kernel: it must stay valid and unchanged until then (orbx_synchronize, or an event on the handle's stream).  The
 * Python wrapper holds a reference to the input of its last device call for this reason; C callers keep the buffer themselves.
 * LATE COPY: the padded level 0 is written late, from d_imgs, by the calls that hand out or read the handle's level 0
 * (orbx_pyramid_level_device / _copy, orbx_debug_blur_copy, orbx_stereo_match, orbx_stereo_match_batch_device): until
 * then d_imgs of the LAST call must stay valid and unchanged as well.  A caller that cannot promise that sets ORBX_LEVEL0_INPLACE=0
 * in the environment before the handle is configured (the copy is then written during the call, as for every other input).
 * A handle whose stereo match needed the late copy writes it during the call from then on.  No load of the in-place
 * kernels leaves [frame, frame + (height - 1) * stride + width) of its frame. */
orbx_status orbx_extract_batch_device(orbx_handle *h, int nframes, const uint8_t *d_imgs, int width,
                                      int height, int stride, int64_t frame_stride,
                                      orbx_keypoint *d_kps, uint8_t *d_desc, int32_t *d_counts,
                                      int32_t *d_status, int cap);

/* Pixel format of the frames given to the three extract entry points (default ORBX_FMT_GRAY8).  The colour formats
 * fuse the cv::cvtColor(CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY) that Tracking::GrabImage* runs before
 * the extractor (src/Tracking.cc:245-271, 302-320, 372-385; mbRGB selects the RGB variants) into level 0:
 * gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14 (OpenCV 3.2, 8-bit).  `stride` stays in bytes, `width` in pixels. */
enum { ORBX_FMT_GRAY8 = 0, ORBX_FMT_RGB8 = 1, ORBX_FMT_BGR8 = 2, ORBX_FMT_RGBA8 = 3, ORBX_FMT_BGRA8 = 4 };
orbx_status orbx_set_input_format(orbx_handle *h, int pixel_format);

/* EuRoC rectification (reference Examples/Stereo/stereo_euroc.cc:126-194): cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR)
 * with the CV_32F maps of cv::initUndistortRectifyMap is fused into level 0; the extract entry points then take the RAW
 * image.  map_x / map_y: width x height floats, row major (M1l / M2l); raw and rectified images have the same size, as in
 * the reference's EuRoC driver.  OpenCV 3.2 fixed-point arithmetic (5-bit fractions, 2^15 weights, border value 0): parity
 * unpinned.  NULL, NULL switches it off.  8-bit gray input only.
 * Map entries: s = cvRound(map * 32) as OpenCV's 32-bit conversion does it -- half to even; NaN, +-inf and every product
 * outside [-2^31, 2^31) give INT_MIN -- then i = saturate_cast<short>(s >> 5), f = s & 31 (include/orbx_rect_digest.h).  An
 * entry that marks an invalid pixel with NaN or inf therefore reads i = -32768: all four taps outside, border value 0. */
orbx_status orbx_set_rectification(orbx_handle *h, const float *map_x, const float *map_y, int width, int height);
/* The digest orbx_set_rectification uploads, for n map entries: out_xy[i] = ix | iy << 16 (int16 each), out_frac[i] =
 * fy << 5 | fx.  Pure host arithmetic: needs no handle and no device; n == 0 writes nothing. */
orbx_status orbx_debug_rect_digest(const float *map_x, const float *map_y, int64_t n, uint32_t *out_xy, uint32_t *out_frac);

/* ---- pyramid access: replaces the public member `mvImagePyramid` (include/ORBextractor.h:185),
 *      read by Frame::ComputeStereoMatches (src/Frame.cc:910,1040,1072,1079).  Valid until the next
 *      extract on this handle ("pyramid is overwritten every frame", include/ORBextractor.h:30-35). -- */
/* width x height of mvImagePyramid[level]: the padded level (sw + 38) x (sh + 38) of a fork handle, the un-padded sw x sh view
 * of an upstream handle (whose 19-pixel reflect-101 border still surrounds it in memory); `pitch` is the same for both */
orbx_status orbx_pyramid_level_info(orbx_handle *h, int level, int *width, int *height, int *pitch);
/* device view of (frame, level): that image, `pitch` bytes per row (after an in-place batch this queues the late
 * level-0 copy on the handle's stream first, see orbx_extract_batch_device) */
orbx_status orbx_pyramid_level_device(orbx_handle *h, int frame, int level, const uint8_t **d_ptr);
/* copies that image into dst (dst_stride >= width) */
orbx_status orbx_pyramid_level_copy(orbx_handle *h, int frame, int level, uint8_t *dst, int dst_stride);

/* ---- matching: ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:2073-2093) evaluated for every
 *      (query, train) pair with the best / second-best bookkeeping of the search loops
 *      (e.g. src/ORBmatcher.cc:627-640).  Device pointers, asynchronous on the handle's stream.
 *      npairs independent problems: pair p uses query rows d_q + p*q_stride (nq[p] rows) and train
 *      rows d_t + p*t_stride (nt[p] rows); outputs [npairs][out_stride].  Contract: out_stride is the
 *      query capacity -- queries beyond it are ignored (nq[p] is clamped to out_stride on the device,
 *      nothing is written outside row p of the outputs).  Train rows: at most 2^20 = 1 048 576 per pair
 *      -- nt[p] is clamped to that on the device and rows beyond it are ignored (a result packs the
 *      train index into 20 bits below the distance), so best_idx never exceeds 2^20 - 1. -------------- */
orbx_status orbx_match_bruteforce_device(orbx_handle *h, int npairs, const uint8_t *d_q,
                                         const int32_t *d_nq, int64_t q_stride, const uint8_t *d_t,
                                         const int32_t *d_nt, int64_t t_stride, int32_t *d_best_idx,
                                         int32_t *d_best_dist, int32_t *d_second_dist, int out_stride);
/* host convenience: one problem, host buffers */
orbx_status orbx_match_bruteforce(orbx_handle *h, const uint8_t *q, int nq, const uint8_t *t, int nt,
                                  int32_t *best_idx, int32_t *best_dist, int32_t *second_dist);
/* full nq x nt distance matrix (uint16), for host-side sequential policies */
orbx_status orbx_hamming_matrix(orbx_handle *h, const uint8_t *q, int nq, const uint8_t *t, int nt,
                                uint16_t *dist);

/* ---- matcher policies on the path ------------------------- */
/* Frame::AssignFeaturesToGrid + PosInGrid (src/Frame.cc:432-460, 729-745): 64 x 48 buckets over keypoints that the
 * caller keeps alive; bounds = mnMinX, mnMaxX, mnMinY, mnMaxY.  Host-side utility (the reference's own form); every policy
 * entry point below builds and queries the grid ON THE DEVICE instead (orbx_grid_build_device / orbx_gated_candidates). */
typedef struct orbx_grid orbx_grid;
orbx_grid *orbx_grid_create(const orbx_keypoint *kps, int n, float min_x, float max_x, float min_y, float max_y);
void orbx_grid_destroy(orbx_grid *g);
/* Frame::GetFeaturesInArea (src/Frame.cc:633-717); returns the number of hits (may exceed cap), < 0 on error */
int orbx_grid_query(const orbx_grid *g, float x, float y, float r, int min_level, int max_level, int32_t *out, int cap);
/* ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:2026-2068) */
void orbx_three_maxima(const int32_t *sizes, int L, int *ind1, int *ind2, int *ind3);
/* ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:570-712; caller src/Tracking.cc:950-962).
 * F1 = (k1, d1, n1), F2 = (k2, d2, n2), bounds4 = {mnMinX, mnMaxX, mnMinY, mnMaxY} of F2,
 * prev_matched[2*n1] = vbPrevMatched (in/out), matches12[n1] = vnMatches12 (out).  Host buffers. */
orbx_status orbx_search_for_initialization(orbx_handle *h, const orbx_keypoint *k1, const uint8_t *d1, int n1,
                                           const orbx_keypoint *k2, const uint8_t *d2, int n2, const float *bounds4,
                                           float *prev_matched, int window, float nnratio, int check_orientation,
                                           int32_t *matches12, int *nmatches);
/* Frame::ComputeStereoMatches (src/Frame.cc:880-1176).  hl / hr are the left / right extractors whose pyramids of
 * (frame_left, frame_right) are still resident (mvImagePyramid is read at :910,1040,1072,1079); keypoints and
 * descriptors are host buffers; u_right / depth = mvuRight / mvDepth.  The reference's unchecked row index (F6)
 * is clamped (on ORBX_PYRAMID_UPSTREAM handles every keypoint row lies inside the table and F6 does not arise).  Both
 * handles must have the same pyramid_mode (ORBX_BAD_ARGUMENT otherwise), here and in the batched call; the behaviour of
 * Frame.cc itself (:1067, the median cut) is the fork's in both modes. */
orbx_status orbx_stereo_match(orbx_handle *hl, orbx_handle *hr, int frame_left, int frame_right,
                              const orbx_keypoint *kl, const uint8_t *dl, int nl, const orbx_keypoint *kr,
                              const uint8_t *dr, int nr, float mb, float mbf, float *u_right, float *depth,
                              int *nmatches);

/* Batched, device-resident form: pair p = frame p of the last orbx_extract_batch_device of `hl` (left eyes) and of `hr`
 * (right eyes); d_k* / d_d* / d_n* are the device buffers those calls filled, `cap` records apart.  Outputs (device):
 * u_right / depth [npairs][cap], nmatches [npairs].  The median cut of :1160-1175 runs on the device too.  Asynchronous on
 * hl's stream.  hl == hr is allowed: the two eyes then went through ONE orbx_extract_batch_device call of 2 * npairs images
 * on that handle, left images first (frames 0 .. npairs-1), right images after them (the reference's two extractors carry the
 * same parameters in stereo, src/Tracking.cc; one batch halves the launches per stereo frame). */
orbx_status orbx_stereo_match_batch_device(orbx_handle *hl, orbx_handle *hr, int npairs, const orbx_keypoint *d_kl,
                                           const uint8_t *d_dl, const int32_t *d_nl, const orbx_keypoint *d_kr,
                                           const uint8_t *d_dr, const int32_t *d_nr, int cap, float mb, float mbf,
                                           float *d_u_right, float *d_depth, int32_t *d_nmatches);

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (src/ORBmatcher.cc:1702-1871;
 * caller Tracking::TrackWithMotionModel, src/Tracking.cc:1430,1445).  The Frame / MapPoint fields the policy reads are
 * passed as arrays.  CurrentFrame.mvpMapPoints is all-NULL on entry (src/Tracking.cc:1420 fills it); the result is
 * matched_last[i2] = index of the last-frame feature whose MapPoint was assigned to current feature i2, or -1. */
typedef struct orbx_frame_view {
    const orbx_keypoint *keys_un;   /* mvKeysUn */
    const uint8_t *desc;            /* mDescriptors, n x 32 */
    const float *u_right;           /* mvuRight (-1 for monocular points) */
    int32_t n;
    float Tcw[16];                  /* mTcw, row major 4x4 */
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y; /* mnMinX .. mnMaxY */
    float mb, mbf;
} orbx_frame_view;
typedef struct orbx_last_frame_view {
    const orbx_keypoint *keys_un;   /* LastFrame.mvKeysUn (octave, angle) */
    int32_t n;
    const uint8_t *has_map_point;   /* mvpMapPoints[i] != NULL && !mvbOutlier[i] */
    const float *world_pos;         /* pMP->GetWorldPos(), 3 floats per feature */
    const uint8_t *mp_desc;         /* pMP->GetDescriptor(), 32 bytes per feature */
    const int32_t *observations;    /* pMP->Observations() */
    float Tcw[16];                  /* LastFrame.mTcw */
} orbx_last_frame_view;
orbx_status orbx_search_by_projection_frame(orbx_handle *h, const orbx_frame_view *cur, const orbx_last_frame_view *last,
                                            float th, int mono, int check_orientation, int32_t *matched_last,
                                            int *nmatches);

/* ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th) (src/ORBmatcher.cc:69-184; caller
 * Tracking::SearchLocalPoints, src/Tracking.cc:1953).  MapPoint fields (written by Frame::isInFrustum in the reference)
 * as arrays; frame_observations[idx] = Observations() of the MapPoint already attached to feature idx, -1 if none.
 * assigned[idx] = index of the MapPoint newly attached to feature idx, or -1.  Only frame->keys_un/desc/u_right/n and
 * the bounds of `frame` are read. */
typedef struct orbx_mappoint_view {
    int32_t n;
    const uint8_t *in_view;       /* mbTrackInView && !isBad() */
    const float *proj;            /* mTrackProjX, mTrackProjY, mTrackProjXR: 3 floats per point */
    const int32_t *level;         /* mnTrackScaleLevel */
    const float *view_cos;        /* mTrackViewCos */
    const uint8_t *desc;          /* GetDescriptor(), 32 bytes per point */
    const int32_t *observations;  /* Observations() */
} orbx_mappoint_view;
orbx_status orbx_search_by_projection_mappoints(orbx_handle *h, const orbx_frame_view *frame,
                                                const int32_t *frame_observations, const orbx_mappoint_view *mps,
                                                float th, float nnratio, int32_t *assigned, int *nmatches);

/* Batched, device-resident forms of the two tracking matchers above: nproblems problems in one call, asynchronous on the
 * handle's stream.  The current frames are read where the device batch left them: d_keys_un / d_desc / d_u_right / d_counts are
 * the buffers of orbx_extract_batch_device, orbx_undistort_keypoints_device and orbx_stereo_match_batch_device or
 * orbx_rgbd_depth_device (nframes frames, records `cap` apart; d_u_right == NULL: every feature monocular, -1), d_cell_begin /
 * d_items the grids orbx_grid_build_device built over them with the same bounds4 and cap.  Problem k names its current frame;
 * several problems may name the same one (TrackWithMotionModel's retry with 2 * th is a second call).  Only the small host-side
 * state of each problem is uploaded -- all problems' arrays through one page-locked staging block, consumed before the call
 * returns -- and only the results are written, on the device: row k of the output ([nproblems][cap]) and d_nmatches[k].  The
 * first min(count[frame], cap) entries of row k and d_nmatches[k] are bit for bit what the single call returns for that
 * frame's keypoints, descriptors and u_right and the same views, in both fp_modes; entries past the frame's count are not
 * written.  The candidate search, the order-dependent selection and the rotation check all run on the device (k_track_project,
 * k_track_cand, k_track_select); no result is waited for (the host waits only where the staging block or the device arena has
 * to grow, or where the upload of the previous call of this kind has not left the staging block yet).  A call of ONE problem is
 * slower than the single call (the ordered pass is one wave per problem): the calls pay off from a few problems on, DESIGN.md
 * section 6.0t.  Everything is validated before any device work: ORBX_BAD_ARGUMENT for
 * nproblems < 0, a null field of a non-empty view, a frame outside [0, nframes), cap <= 0, or an octave / level outside
 * [0, nlevels) on a point that has a MapPoint / is in view; ORBX_UNSUPPORTED for cap > 65535.  nproblems == 0 launches nothing. */
typedef struct orbx_track_frame_problem {
    int32_t frame;                  /* CurrentFrame = this frame of the device batch */
    float th;
    int32_t mono;                   /* bMono */
    float Tcw[16];                  /* CurrentFrame.mTcw, row major 4x4 */
    orbx_last_frame_view last;      /* host arrays */
} orbx_track_frame_problem;
/* camera4 = fx, fy, cx, cy; bounds4 = mnMinX, mnMaxX, mnMinY, mnMaxY; mb, mbf as orbx_frame_view */
orbx_status orbx_search_by_projection_frame_batch_device(orbx_handle *h, int nproblems, const orbx_track_frame_problem *problems,
                                                         int nframes, const orbx_keypoint *d_keys_un, const uint8_t *d_desc,
                                                         const float *d_u_right, const int32_t *d_counts, int cap,
                                                         const int32_t *d_cell_begin, const uint16_t *d_items,
                                                         const float *camera4, const float *bounds4, float mb, float mbf,
                                                         int check_orientation, int32_t *d_matched_last, int32_t *d_nmatches);
typedef struct orbx_track_points_problem {
    int32_t frame;
    float th;
    const int32_t *frame_observations;  /* host, cap entries (those past the frame's count are ignored); NULL: all -1 */
    orbx_mappoint_view points;          /* host arrays */
} orbx_track_points_problem;
orbx_status orbx_search_by_projection_mappoints_batch_device(orbx_handle *h, int nproblems,
                                                             const orbx_track_points_problem *problems, int nframes,
                                                             const orbx_keypoint *d_keys_un, const uint8_t *d_desc,
                                                             const float *d_u_right, const int32_t *d_counts, int cap,
                                                             const int32_t *d_cell_begin, const uint16_t *d_items,
                                                             const float *bounds4, float nnratio, int32_t *d_assigned,
                                                             int32_t *d_nmatches);

/* MapPoint::PredictScale(currentDist, Frame*) (src/MapPoint.cc:706-721) without a logarithm at run time.  The level
 *   nScale = (int)ceilf(logf(ratio) / logf(scaleFactor)), clamped to [0, nlevels - 1],  ratio = mfMaxDistance / currentDist
 * is a non-decreasing step function of the float `ratio`.  orbx_create finds, with the host's own libm and by bisection over the
 * float bit patterns, thr[k] = the smallest positive finite float for which the expression gives >= k (k = 1 .. nlevels - 1;
 * +inf where no finite float does); the level is the number of k with ratio >= thr[k].  The caller's reference code runs in the
 * same process against the same libm, so the two agree wherever that libm's logf is monotone.
 * OUTSIDE the parity contract: ratio = NaN, <= 0 or +inf (currentDist == 0, a non-positive mfMaxDistance) is a float -> int
 * conversion with undefined behaviour in the reference; here the table rule applies as it stands -- NaN and <= 0 give 0, +inf
 * gives nlevels - 1 -- and nothing faults.  Both are host functions and work on a host-only handle.
 * orbx_predict_scale_table: thr holds n >= nlevels floats; thr[0] = 0 (not used), thr[1 .. nlevels - 1] as above.
 * orbx_predict_scale: the level; -1 without a handle. */
orbx_status orbx_predict_scale_table(const orbx_handle *h, float *thr, int n);
int orbx_predict_scale(const orbx_handle *h, float max_distance, float current_dist);

/* Tracking::SearchLocalPoints (src/Tracking.cc:1875-1955) for many (frame, pose, local map) problems in one call: per point
 * Frame::isInFrustum (src/Frame.cc:529-620) with MapPoint::PredictScale, then SearchByProjection(F, vpMapPoints, th), all on the
 * device (k_track_frustum, then k_track_cand and k_track_select exactly as orbx_search_by_projection_mappoints_batch_device
 * runs them).  The local map is ONE pool per call, uploaded once and shared by all problems; a problem names its points as pool
 * indices in list order and carries its pose.  The frustum stage evaluates the reference's expressions in its order: Pc = Rcw P +
 * tcw (cv::gemm's float special case), PcZ < 0, invz = 1.0f / PcZ (a float division), u = fx PcX invz + cx and v likewise and
 * ur = u - mbf invz (contracted under ORBX_FP_GCC_FMA as in orbx_search_by_projection_frame, separate roundings under
 * ORBX_FP_STRICT), the four bounds tests, dist = (float)sqrt of the double sum of squares of P - Ow against [0.8f min, 1.2f max],
 * viewCos = (float)(double dot / dist) against viewing_cos_limit, the level of orbx_predict_scale(max_distance, dist), and the
 * matcher's window r = (viewCos > 0.998 ? 2.5f : 4.0f) (* th where th != 1.0) * mvScaleFactors[level] with the level band
 * [level - 1, level].  The cv::Mat sums and cv::norm are OpenCV-owned arithmetic: parity with a particular OpenCV build is not
 * pinned there (as for orbx_search_by_projection_frame).
 * Contract of the two calls above: asynchronous on the handle's stream, one page-locked staging block consumed before the call
 * returns, nothing downloaded.  d_assigned ([nproblems][cap]) and d_nmatches are what
 * orbx_search_by_projection_mappoints_batch_device writes for the same frames when it is fed this stage's results.
 * d_in_view[q] (q = the point's position in the concatenation of all problems' lists; may be NULL) = mbTrackInView, which the
 * caller needs for IncreaseVisible() and nToMatch; d_track[q] (may be NULL) = the MapPoint's tracking fields, written only where
 * d_in_view[q] would be 1.  Validated before any device work: ORBX_BAD_ARGUMENT for nproblems < 0, a null field of a non-empty
 * pool, a null map with a non-empty problem, an index outside the pool, a frame outside [0, nframes), cap <= 0;
 * ORBX_UNSUPPORTED for cap > 65535.  nproblems == 0 launches nothing; an empty pool (every problem then has npoints == 0)
 * launches nothing that reads it. */
typedef struct orbx_local_map_view {      /* one pool per call, uploaded once, shared by all problems */
    int32_t n;
    const float *world_pos;               /* GetWorldPos(), 3 per point */
    const float *normal;                  /* GetNormal(), 3 per point */
    const float *min_distance;            /* mfMinDistance (raw; the 0.8f is applied here) */
    const float *max_distance;            /* mfMaxDistance (raw; the 1.2f is applied here, PredictScale uses it raw) */
    const uint8_t *desc;                  /* GetDescriptor(), 32 per point */
    const int32_t *observations;          /* Observations() */
} orbx_local_map_view;
typedef struct orbx_track_local_problem {
    int32_t frame;                        /* this frame of the device batch */
    float th;
    float viewing_cos_limit;              /* 0.5f in Tracking::SearchLocalPoints */
    float Tcw[16];                        /* mTcw, row major 4x4 (mRcw, mtcw are read from it) */
    float Ow[3];                          /* mOw as the Frame holds it */
    int32_t npoints;
    const int32_t *point_index;           /* mvpLocalMapPoints as pool indices, in list order; NULL: the whole pool in order
                                             (npoints must then equal the pool's n) */
    const uint8_t *skip;                  /* npoints: mnLastFrameSeen == mnId || isBad(); NULL: none */
    const int32_t *frame_observations;    /* as orbx_track_points_problem */
} orbx_track_local_problem;
typedef struct orbx_track_state { float proj_x, proj_y, proj_xr, view_cos; int32_t level; } orbx_track_state;
orbx_status orbx_search_local_points_batch_device(orbx_handle *h, int nproblems, const orbx_track_local_problem *problems,
                                                  const orbx_local_map_view *map, int nframes,
                                                  const orbx_keypoint *d_keys_un, const uint8_t *d_desc, const float *d_u_right,
                                                  const int32_t *d_counts, int cap, const int32_t *d_cell_begin,
                                                  const uint16_t *d_items, const float *camera4, const float *bounds4, float mbf,
                                                  float nnratio, int32_t *d_assigned, int32_t *d_nmatches, uint8_t *d_in_view,
                                                  orbx_track_state *d_track);

/* ---- MapPoint::ComputeDistinctiveDescriptors / MapPoint::UpdateNormalAndDepth for the loops that end with them
 * (LocalMapping::ProcessNewKeyFrame, CreateNewMapPoints, SearchInNeighbors, LoopClosing::CorrectLoop, the keyframe insertion of
 * Tracking): inside these loops the points are independent, so one ragged batch equals the loop.  Point p owns the rows
 * obs_begin[p] .. obs_begin[p + 1] (obs_begin[0] == 0, npoints + 1 entries, not decreasing); N is their count.
 *
 * Descriptors (src/MapPoint.cc:468-515; kernels k_mp_distinct for N <= 16, four points per wave, and k_mp_distinct_wide, one
 * workgroup per point, for every other N): D[i][j] = popcount(row i ^ row j), D[i][i] = 0 belongs to row i; median_i = element
 * (N - 1) / 2 of row i sorted ascending; best_idx = the FIRST i with the smallest median.  The rows are those of the caller's
 * std::map<KeyFrame*, size_t> in ITS iteration order with the bad keyframes already left out: the order decides between equal
 * medians, so it is part of the contract.  N == 0: best_idx = best_median = -1 and the best_desc row is left as it was.
 * best_median and best_desc may be NULL.  The _device form names the rows instead of copying them: row t is
 * d_pool[obs_row[t]], d_pool a device buffer of pool_rows x 32 bytes, 16-byte aligned, whose contents are complete with respect to the handle's
 * stream when the call is made; the results still land on the host.
 *
 * Normal and depth (src/MapPoint.cc:570-638 with cv::Mat's arithmetic as tests/compat_runtime/opencv2/core/core.hpp states it;
 * kernel k_mp_normal_depth, sixteen lanes per point): for every row in order, bad keyframes INCLUDED, d = pos - center (float),
 * nrm = sqrt(d.d) summed in double in element order, normal = normal + (float)((double)d / nrm) one float addition per row in
 * row order; then dist = (float)norm(pos - ref_center), max_distance = dist * mvScaleFactors[ref_level], min_distance =
 * max_distance / mvScaleFactors[nlevels - 1], normal = (float)((double)normal / (double)N).  The scale factors are the
 * handle's (orbx_get_scale_tables).  No multiply-add pair occurs: both fp_modes give the same bits.  N == 0: the point's
 * normal / min_distance / max_distance are left as they were and its ref_level is not looked at.
 *
 * All three: synchronous, on the handle's stream; one upload from one page-locked block, the launches, one download.
 * Validated before any device work (a host-only handle can be used to test a call): ORBX_BAD_ARGUMENT for npoints < 0, a NULL
 * required pointer, obs_begin[0] != 0 or a decreasing obs_begin, pool_rows < 0, an obs_row outside [0, pool_rows), a d_pool
 * that is not 16-byte aligned, a ref_level outside [0, nlevels) on a point with rows.  npoints == 0 succeeds and does nothing;
 * well-formed input on a host-only handle returns ORBX_NO_DEVICE. */
orbx_status orbx_distinctive_descriptors_batch(orbx_handle *h, int npoints, const int32_t *obs_begin, const uint8_t *desc,
                                               int32_t *best_idx, int32_t *best_median, uint8_t *best_desc);
orbx_status orbx_distinctive_descriptors_batch_device(orbx_handle *h, const uint8_t *d_pool, int64_t pool_rows, int npoints,
                                                      const int32_t *obs_begin, const int64_t *obs_row, int32_t *best_idx,
                                                      int32_t *best_median, uint8_t *best_desc);
orbx_status orbx_update_normal_and_depth_batch(orbx_handle *h, int npoints, const int32_t *obs_begin, const float *pos,
                                               const float *centers, const float *ref_center, const int32_t *ref_level,
                                               float *normal, float *min_distance, float *max_distance);

/* ---- BoW-guided policies.  Host code keeps the pointer chasing (KeyFrame / MapPoint /
 * DBoW2 containers) and hands the fields the policies read as arrays; the Hamming distances come from the GPU, the
 * order-dependent selection runs on the host exactly as the reference does. */
/* DBoW2::FeatureVector = std::map<NodeId, std::vector<unsigned int>> (Thirdparty/DBoW2/DBoW2/FeatureVector.h), flattened
 * in map order: node ids strictly ascending, n_nodes + 1 offsets into `index`, feature indices in each vector's order. */
typedef struct orbx_featvec_view {
    int32_t n_nodes;
    const uint32_t *node_id;
    const int32_t *begin;
    const uint32_t *index;
} orbx_featvec_view;
typedef struct orbx_keyframe_view {
    const orbx_keypoint *keys_un;    /* mvKeysUn */
    const uint8_t *desc;             /* mDescriptors, n x 32 */
    int32_t n;
    const uint8_t *has_map_point;    /* GetMapPoint(i) != NULL && !isBad() */
    const float *u_right;            /* mvuRight (SearchForTriangulation only) */
    orbx_featvec_view feat_vec;      /* mFeatVec */
    const float *scale_factors;      /* mvScaleFactors, per octave (SearchForTriangulation: second keyframe) */
    const float *level_sigma2;       /* mvLevelSigma2, per octave (SearchForTriangulation: second keyframe) */
} orbx_keyframe_view;
/* ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches) (src/ORBmatcher.cc:248-410;
 * callers Tracking::TrackReferenceKeyFrame src/Tracking.cc:1281, Relocalization :2115).  f_keys = F.mvKeys (angle only).
 * matched_kf[i] = index of the keyframe feature whose MapPoint is vpMapPointMatches[i], -1 = NULL. */
orbx_status orbx_search_by_bow_keyframe_frame(orbx_handle *h, const orbx_keyframe_view *kf, const orbx_keypoint *f_keys,
                                              const uint8_t *f_desc, int nf, const orbx_featvec_view *f_feat_vec,
                                              float nnratio, int check_orientation, int32_t *matched_kf, int *nmatches);
/* ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12) (:722-866; caller
 * LoopClosing::ComputeSim3).  matches12[i1] = index of the KF2 feature whose MapPoint is vpMatches12[i1], -1 = NULL. */
orbx_status orbx_search_by_bow_keyframes(orbx_handle *h, const orbx_keyframe_view *kf1, const orbx_keyframe_view *kf2,
                                         float nnratio, int check_orientation, int32_t *matches12, int *nmatches);
/* Batched forms of the two calls above for the loops that run them once per candidate keyframe.  The iterations of those
 * loops are independent (each writes only its own vvpMapPointMatches[i]), and with every feature index held at most once
 * per feature vector the reference's selection is order-dependent only inside one vocabulary node: the selection runs on
 * the device, one wave per (problem, common node), the rotation check one workgroup per problem.  One upload, one
 * download.  Views of more than 65535 features return ORBX_UNSUPPORTED (16-bit positions inside a node). */
/* Tracking::Relocalization (src/Tracking.cc:2283-2300): SearchByBoW(kfs[k], F) for k < nproblems.  matched_kf[k] (nf entries)
 * and nmatches[k] are exactly what orbx_search_by_bow_keyframe_frame returns for (kfs[k], F).  Every feature vector must
 * hold each feature index at most once (true of DBoW2::transform); otherwise ORBX_BAD_ARGUMENT. */
orbx_status orbx_search_by_bow_keyframe_frame_batch(orbx_handle *h, int nproblems, const orbx_keyframe_view *const *kfs,
        const orbx_keypoint *f_keys, const uint8_t *f_desc, int nf, const orbx_featvec_view *f_feat_vec,
        float nnratio, int check_orientation, int32_t *const *matched_kf, int *nmatches);
/* LoopClosing::ComputeSim3 (src/LoopClosing.cc:440-466): SearchByBoW(kf1, kf2[k]); matches12[k] (kf1->n entries) and
 * nmatches[k] exactly as orbx_search_by_bow_keyframes(kf1, kf2[k]).  Same feature-vector rule. */
orbx_status orbx_search_by_bow_keyframes_batch(orbx_handle *h, const orbx_keyframe_view *kf1, int nproblems,
        const orbx_keyframe_view *const *kf2, float nnratio, int check_orientation, int32_t *const *matches12, int *nmatches);
/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (:879-1087, CheckDistEpipolarLine
 * :206-233; caller LocalMapping::CreateNewMapPoints).  F12: row-major 3x3; (ex, ey): epipole of KF1's centre in KF2
 * (:892-898, computed by the caller from its pose matrices).  vMatchedPairs = (i1, matches12[i1]) for ascending i1 with
 * matches12[i1] >= 0.  The handle's fp_mode selects the contraction of the float expressions. */
orbx_status orbx_search_for_triangulation(orbx_handle *h, const orbx_keyframe_view *kf1, const orbx_keyframe_view *kf2,
                                          const float *F12, float ex, float ey, int only_stereo, int check_orientation,
                                          int32_t *matches12, int *nmatches);
/* The loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:375-430) calls SearchForTriangulation for the current keyframe
 * against each covisible neighbour and creates MapPoints for the matches before it goes on to the next neighbour.  The Hamming
 * distances depend on descriptors and feature vectors only: _create computes them for ALL neighbours in one device round trip;
 * _select runs the reference's selection for neighbour k on the host with the has_map_point flags the views carry WHEN IT IS
 * CALLED (same keyframes, same feature counts as at _create): the matches of K single calls for one ~60 us round trip. */
typedef struct orbx_triangulation_batch orbx_triangulation_batch;
orbx_status orbx_triangulation_batch_create(orbx_handle *h, const orbx_keyframe_view *kf1, int nproblems,
                                            const orbx_keyframe_view *const *kf2, orbx_triangulation_batch **out);
orbx_status orbx_triangulation_batch_select(const orbx_triangulation_batch *b, int k, const orbx_keyframe_view *kf1,
                                            const orbx_keyframe_view *kf2, const float *F12, float epipole_x, float epipole_y,
                                            int only_stereo, int check_orientation, int32_t *matches12, int *nmatches);
void orbx_triangulation_batch_destroy(orbx_triangulation_batch *b);

/* ---- projection-guided back-end policies.  The pose algebra in front of them (cv::Mat products, cv::norm,
 * MapPoint::PredictScale: OpenCV / libm code) stays in the maintainer's shim, which IS the reference's code; the entry
 * points start where the reference holds, for every MapPoint, "passed every geometric test", the projection, the
 * predicted level and the representative descriptor. */
typedef struct orbx_projected_points {
    int32_t n;
    const uint8_t *valid;     /* the point reaches `const float radius = th * ...` in the reference */
    const float *uv;          /* projection (u, v), 2 floats per point */
    const float *u_right;     /* ur = u - bf * invz (orbx_fuse only) */
    const int32_t *level;     /* nPredictedLevel */
    const uint8_t *desc;      /* pMP->GetDescriptor(), 32 bytes per point */
    const float *angle;       /* pKF->mvKeysUn[i].angle (orbx_search_by_projection_keyframe with check_orientation) */
} orbx_projected_points;
/* Every projection-guided entry point below gates its candidates on the device with 16-bit feature indices: a target with more
 * than 65535 features returns ORBX_UNSUPPORTED (ORB-SLAM2 frames carry 1000-4000). */
typedef struct orbx_target_view {   /* the KeyFrame / Frame whose features are searched */
    const orbx_keypoint *keys_un;    /* mvKeysUn */
    const uint8_t *desc;             /* mDescriptors */
    const float *u_right;            /* mvuRight (orbx_fuse only) */
    int32_t n;
    float min_x, max_x, min_y, max_y; /* mnMinX .. mnMaxY (grid of GetFeaturesInArea) */
    const float *scale_factors;      /* mvScaleFactors */
    const float *inv_level_sigma2;   /* mvInvLevelSigma2 (orbx_fuse only) */
} orbx_target_view;
/* ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th) (src/ORBmatcher.cc:1100-1280), lines
 * :1168-1245: best_idx[i] = keyframe feature the point is fused into, -1 = none.  The caller then runs the Replace /
 * AddObservation / AddMapPoint branch (:1248-1275) over i in order; it does not feed back into the selection. */
orbx_status orbx_fuse(orbx_handle *h, const orbx_target_view *kf, const orbx_projected_points *pts, float th,
                      int32_t *best_idx, int *nfused);
/* ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint) (:1282-1430), lines :1345-1400 */
orbx_status orbx_fuse_sim3(orbx_handle *h, const orbx_target_view *kf, const orbx_projected_points *pts, float th,
                           int32_t *best_idx, int *nfused);
/* Batched forms: nproblems (target, point set) pairs through ONE upload, ONE grid-build + gate launch pair and ONE download
 * instead of a ~60 us synchronous round trip each.  The reference calls Fuse once per neighbour keyframe in a loop --
 * LocalMapping::SearchInNeighbors (src/LocalMapping.cc:750-768), LoopClosing::SearchAndFuse -- and that loop is the batch.
 * best_idx[k][i], nfused[k] are exactly what orbx_fuse / orbx_fuse_sim3 return for (kfs[k], pts[k]); all targets must share the
 * image bounds (min_x .. max_y: Frame's static mnMinX .. mnMaxY).  Earlier iterations of the reference's loop reach later ones
 * only through pMP->isBad() / IsInKeyFrame(), which the caller re-checks while it applies the results in order. */
orbx_status orbx_fuse_batch(orbx_handle *h, int nproblems, const orbx_target_view *const *kfs,
                            const orbx_projected_points *const *pts, float th, int32_t *const *best_idx, int *nfused);
orbx_status orbx_fuse_sim3_batch(orbx_handle *h, int nproblems, const orbx_target_view *const *kfs,
                                 const orbx_projected_points *const *pts, float th, int32_t *const *best_idx, int *nfused);
/* ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, vpPoints, vpMatched, int th) (:415-560), lines :498-556.
 * matched[idx] = vpMatched[idx] != NULL, updated exactly as the reference updates vpMatched (point order matters);
 * best_idx[i] = feature that received point i, -1 = none. */
orbx_status orbx_search_by_projection_sim3(orbx_handle *h, const orbx_target_view *kf, const orbx_projected_points *pts,
                                           int th, uint8_t *matched, int32_t *best_idx, int *nmatches);
/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (:1433-1690) from the two projection loops on.
 * pts1_in_2: one entry per KF1 feature (valid = has a good MapPoint, !vbAlreadyMatched1, all geometric tests), projected
 * into KF2; pts2_in_1 the converse.  matches12[i1] = KF2 feature whose MapPoint becomes vpMatches12[i1], -1 otherwise. */
orbx_status orbx_search_by_sim3(orbx_handle *h, const orbx_target_view *kf1, const orbx_target_view *kf2,
                                const orbx_projected_points *pts1_in_2, const orbx_projected_points *pts2_in_1, float th,
                                int32_t *matches12, int *nfound);
/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist) (:1873-2020; caller
 * Tracking::Relocalization).  pts = pKF's MapPoints; cur_has_map_point[i2] = CurrentFrame.mvpMapPoints[i2] != NULL
 * (in/out); matched_point[i2] = index of the point attached to feature i2, -1. */
orbx_status orbx_search_by_projection_keyframe(orbx_handle *h, const orbx_target_view *cur, const orbx_projected_points *pts,
                                               float th, int orb_dist, int check_orientation, uint8_t *cur_has_map_point,
                                               int32_t *matched_point, int *nmatches);

/* ---- DBoW2 transform: Frame::ComputeBoW (src/Frame.cc:750-765) =
 * TemplatedVocabulary<FORB>::transform(features, BowVector&, FeatureVector&, 4)
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1136-1216, 1240-1285; FORB::distance FORB.cpp:81-101). */
typedef struct orbx_vocabulary_view {   /* m_nodes flattened; node 0 is the root */
    int32_t n_nodes, k, L;
    int32_t weighting;               /* DBoW2::WeightingType: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY */
    int32_t scoring;                 /* DBoW2::ScoringType: 0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA, 5 DOT_PRODUCT */
    const int32_t *child_begin;      /* n_nodes + 1 offsets into child_ids: Node::children in vector order */
    const uint32_t *child_ids;       /* every child id is greater than its parent's (true of every DBoW2-built tree) */
    const uint8_t *desc;             /* Node::descriptor, n_nodes x 32 (the root's row is not read) */
    const double *weight;            /* Node::weight */
    const uint32_t *word_id;         /* Node::word_id (meaningful for leaves) */
} orbx_vocabulary_view;
typedef struct orbx_vocabulary orbx_vocabulary;
/* copies the tree to the handle's device; the vocabulary can then be used with any handle on that device.  It keeps the
 * handle's fp_mode for orbx_bow_vectors.  A host-only handle (device = -2) gets the host tables alone: orbx_bow_vectors and
 * orbx_vocabulary_scoring work, the transform calls refuse it. */
orbx_status orbx_vocabulary_create(orbx_handle *h, const orbx_vocabulary_view *view, orbx_vocabulary **out);
void orbx_vocabulary_destroy(orbx_vocabulary *voc);
/* per descriptor: transform(feature, word_id, weight, &nid, levelsup).  Host buffers. */
orbx_status orbx_bow_transform(orbx_handle *h, const orbx_vocabulary *voc, const uint8_t *desc, int n, int levelsup,
                               uint32_t *word_id, double *weight, uint32_t *node_id);
/* batched, device buffers (descriptors as orbx_extract_batch_device leaves them): d_leaf_node[f][i] = leaf reached by
 * descriptor i of frame f (word id / weight = tables of the view), d_node_id[f][i] = node at depth L - levelsup */
orbx_status orbx_bow_transform_device(orbx_handle *h, const orbx_vocabulary *voc, int nframes, const uint8_t *d_desc,
                                      const int32_t *d_counts, int64_t desc_frame_stride, int max_n, int levelsup,
                                      uint32_t *d_leaf_node, uint32_t *d_node_id, int out_stride);
/* the BowVector and FeatureVector transform() builds from the per-descriptor results, flattened in map order (bow_word
 * ascending with bow_value; fv_node ascending, fv_begin[n_fv_nodes + 1], fv_index = an orbx_featvec_view).  Capacities: n.
 * The L2 normalisation (scoring L2_NORM) sums `norm += v * v` fused under ORBX_FP_GCC_FMA, as g++ -O3 -mfma compiles
 * BowVector::normalize, and unfused under ORBX_FP_STRICT. */
orbx_status orbx_bow_vectors(const orbx_vocabulary *voc, const uint32_t *word_id, const double *weight,
                             const uint32_t *node_id, int n, uint32_t *bow_word, double *bow_value, int *n_bow,
                             uint32_t *fv_node, int32_t *fv_begin, uint32_t *fv_index, int *n_fv_nodes);

/* ---- Keyframe database (reference src/KeyFrameDatabase.cc, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp): the link between
 * orbx_bow_vectors and the batched SearchByBoW calls.  The database keeps the BowVectors of its entries (on the device for a
 * device handle) and the per-entry state the reference keeps in the KeyFrames: mnRelocQuery / mnRelocWords / mRelocScore and
 * mnLoopQuery / mnLoopWords / mLoopScore.  That state persists across queries exactly as in the reference; DESIGN.md section 2
 * F8 states what a read of a score no query has written yields.  A database needs nothing from the vocabulary but its scoring
 * type (orbx_vocabulary_scoring), so it also works with a host-only handle, where every call runs the reference's
 * inverted-file walk on the host; ORBX_KFDB=host (read per call) selects that path on a device handle too.  KL scoring needs
 * libm's log and exists on the host path only (ORBX_UNSUPPORTED otherwise).  All buffers are host buffers; BowVectors are
 * passed as orbx_bow_vectors writes them (words ascending).  One database serves one thread at a time. */
typedef struct orbx_kfdb orbx_kfdb;
int orbx_vocabulary_scoring(const orbx_vocabulary *voc);   /* the view's scoring field; -1 for NULL */
/* TemplatedVocabulary::score(a, b) for all six scoring types, on the host.  The handle supplies fp_mode: `score += vi * wi`
 * of L2 / dot product (and the products of KL) is one fused multiply-add under ORBX_FP_GCC_FMA. */
orbx_status orbx_bow_score(const orbx_handle *h, int scoring, const uint32_t *a_word, const double *a_value, int na,
                           const uint32_t *b_word, const double *b_value, int nb, double *score);
orbx_status orbx_kfdb_create(orbx_handle *h, int scoring, orbx_kfdb **out);   /* the handle must outlive the database */
void orbx_kfdb_destroy(orbx_kfdb *db);
orbx_status orbx_kfdb_clear(orbx_kfdb *db);
int orbx_kfdb_size(const orbx_kfdb *db);
/* KeyFrameDatabase::add / erase (:56-88).  id = KeyFrame::mnId, unique: a duplicate add or an unknown erase is
 * ORBX_BAD_ARGUMENT.  An entry starts with the state of a new KeyFrame (marks and counts 0, scores unwritten); erase keeps the
 * order of the other entries.  New vectors reach the device pool with the next query (one copy for all of them). */
orbx_status orbx_kfdb_add(orbx_kfdb *db, int64_t id, const uint32_t *bow_word, const double *bow_value, int n);
orbx_status orbx_kfdb_erase(orbx_kfdb *db, int64_t id);
/* mpVocabulary->score(query, entry) for the named entries, one launch: the minScore loop of LoopClosing::DetectLoop
 * (src/LoopClosing.cc:143-157).  Touches no state. */
orbx_status orbx_kfdb_score_entries(orbx_kfdb *db, const uint32_t *q_word, const double *q_value, int nq, const int64_t *ids,
                                    int n, double *scores);
/* Steps 1-3 of DetectRelocalizationCandidates (:274-343) for nqueries frames, as if run one after the other in that order:
 * query q has id query_ids[q] (Frame::mnId) and the BowVector q_word / q_value[q_begin[q] .. q_begin[q + 1]).  Per query:
 * n_matches[q] = length of lScoreAndMatch, min_common_words[q] = minCommonWords (0 when no entry shares a word); the list
 * itself is read with orbx_kfdb_query_matches.  One launch set and one device round trip per call while nqueries x entries
 * stays below 8 M pairs (whole queries per set beyond that); downloads are bounded by the number of sharers. */
orbx_status orbx_kfdb_query_reloc(orbx_kfdb *db, int nqueries, const int64_t *query_ids, const int32_t *q_begin,
                                  const uint32_t *q_word, const double *q_value, int32_t *n_matches, int32_t *min_common_words);
/* Steps 1-3 of DetectLoopCandidates (:114-185): connected_ids = pKF->GetConnectedKeyFrames() (ids outside the database are
 * ignored), lScoreAndMatch keeps si >= min_score. */
orbx_status orbx_kfdb_query_loop(orbx_kfdb *db, int64_t query_id, const uint32_t *q_word, const double *q_value, int nq,
                                 const int64_t *connected_ids, int nconnected, float min_score, int32_t *n_matches,
                                 int32_t *min_common_words);
/* lScoreAndMatch of query `query` of the last query call, in list order; valid until the next add / erase / clear / query */
orbx_status orbx_kfdb_query_matches(orbx_kfdb *db, int query, int64_t *ids, float *scores, int cap, int *n);
/* the entries whose marks / counts / scores that query changed (a drop-in class writes exactly these back to its KeyFrames) */
orbx_status orbx_kfdb_query_touched(orbx_kfdb *db, int query, int64_t *ids, int cap, int *n);
/* Steps 4-5 (:187-263, :345-411) for query `query` of the last query call.  neigh_ids[neigh_begin[i] .. neigh_begin[i + 1]) =
 * GetBestCovisibilityKeyFrames(10) of lScoreAndMatch[i], evaluated by the caller at this moment, as the reference does (ids
 * outside the database carry no mark and are skipped).  It is a second call because the covisibility graph is the caller's
 * state -- the same split as orbx_triangulation_batch_create / _select.  It sees marks, counts and scores as of that query,
 * not as of the end of the batch, so it is called for query 0, 1, ... in order, each at most once, before any other call on the
 * database (ORBX_BAD_ARGUMENT otherwise; queries it is not called for still leave their state behind).  candidates: cap >=
 * n_matches[query].  *n_unscored_reads = reads of a score that no query had written (F8: each read as 0.0f). */
orbx_status orbx_kfdb_select_groups(orbx_kfdb *db, int query, const int32_t *neigh_begin, const int64_t *neigh_ids,
                                    int64_t *candidates, int cap, int *n, int *n_unscored_reads);
/* mn{Reloc,Loop}Query, mn{Reloc,Loop}Words, m{Reloc,Loop}Score of an entry (loop_form = 0 / 1); *score_valid = 0 while no
 * query has written the score (*score is 0.0f then).  Ends the batch of the last query call like add / erase do. */
orbx_status orbx_kfdb_state(orbx_kfdb *db, int64_t id, int loop_form, int64_t *mark, int32_t *words, float *score,
                            int *score_valid);

/* ---- Frame glue: Frame::UndistortKeyPoints / ComputeImageBounds (src/Frame.cc:770-865) =
 * cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) on the keypoint coordinates.  camera4 = fx, fy, cx, cy of mK;
 * dist = mDistCoef (k1, k2, p1, p2[, k3[, k4, k5, k6[, s1, s2, s3, s4[, tauX, tauY]]]], ndist <= 14); the first 12 are
 * evaluated.  The tilted-sensor terms are not implemented: ndist 13 or 14 is accepted only with dist[12] == dist[13] == 0, a
 * non-zero tilt term is ORBX_UNSUPPORTED before any work (here, in orbx_image_bounds, orbx_rgbd_depth_device and
 * orbx_extract_rgbd_batch; outputs untouched).  dist[0] == 0 copies the keypoints unchanged (:772-776).  OpenCV 3.2
 * arithmetic (double precision, five fixed iterations): parity unpinned, like every OpenCV-owned stage.  The device form
 * works on the buffers orbx_extract_batch_device filled (records `cap` apart, counts per frame) so that the keypoints need
 * not leave the GPU; AssignFeaturesToGrid on those buffers is orbx_grid_build_device (below), so a gated match reads them
 * where the extraction left them. */
orbx_status orbx_undistort_keypoints_device(orbx_handle *h, int nframes, const orbx_keypoint *d_kps, const int32_t *d_counts,
                                            int cap, const float *camera4, const float *dist, int ndist,
                                            orbx_keypoint *d_kps_un);
orbx_status orbx_undistort_keypoints(orbx_handle *h, const orbx_keypoint *kps, int n, const float *camera4, const float *dist,
                                     int ndist, orbx_keypoint *kps_un);
/* ---- RGB-D Frame (reference src/Frame.cc:237-321): Frame::ComputeStereoFromRGBD (src/Frame.cc:1179-1226) after the depth
 * conversion of Tracking::GrabImageRGBD (src/Tracking.cc:327-332).  depth_scale = Tracking's mDepthMapFactor (1 / DepthMapFactor
 * of the settings file, 1 if |DepthMapFactor| < 1e-5).  Depth frames are W x H, `stride` bytes per row (>= W * element size,
 * a multiple of it), `frame_stride` bytes apart:
 *   ORBX_DEPTH_U16: convertTo(CV_32F, scale) makes a continuous float image, pixel = (float)raw * scale;
 *   ORBX_DEPTH_F32: with fabs(scale - 1.0f) > 1e-5 converted in place (the caller's stride is kept, bytes between rows stay
 *                   unscaled), otherwise read as they are.
 * Per keypoint: u = (int)kps[i].x, v = (int)kps[i].y (the DISTORTED keypoint: padded-image coordinates on a fork handle, image
 * coordinates on an ORBX_PYRAMID_UPSTREAM handle, where every keypoint lies inside the depth image and F7 does not arise); the
 * sample is byte o = v * pitch + 4 * u of that float image (pitch = 4 * W for u16, `stride` for f32; a u beyond the row wraps
 * into the next row, as in the reference).  F7: o + 4 > (H - 1) * pitch + 4 * W lies past the image's
 * memory and gives no depth, and so do negative, non-finite or too-large coordinates.  d > 0: depth[i] = d,
 * u_right[i] = kps_un[i].x - mbf / d (IEEE single division); otherwise both -1. */
enum { ORBX_DEPTH_U16 = 0, ORBX_DEPTH_F32 = 1 };
/* Device buffers as orbx_extract_batch_device filled them (records `cap` apart, d_counts per frame), fused with
 * orbx_undistort_keypoints_device: one launch computes mvKeysUn (camera4 / dist / ndist as there; written to d_kps_un unless it
 * is NULL, byte-identical to orbx_undistort_keypoints_device), mvuRight and mvDepth ([nframes][cap], rows beyond a frame's
 * count untouched).  Asynchronous on the handle's stream. */
orbx_status orbx_rgbd_depth_device(orbx_handle *h, int nframes, const orbx_keypoint *d_kps, const int32_t *d_counts, int cap,
                                   const float *camera4, const float *dist, int ndist, const void *d_depth, int depth_format,
                                   int width, int height, int stride, int64_t frame_stride, float depth_scale, float mbf,
                                   orbx_keypoint *d_kps_un, float *d_u_right, float *d_depth_out);
/* The body of Frame::ComputeStereoFromRGBD for one frame: host buffers, kps = mvKeys, kps_un = mvKeysUn (as the Frame holds
 * them), depth = the frame's depth image; run on the device like orbx_undistort_keypoints. */
orbx_status orbx_rgbd_depth(orbx_handle *h, const orbx_keypoint *kps, const orbx_keypoint *kps_un, int n, const void *depth,
                            int depth_format, int width, int height, int stride, float depth_scale, float mbf, float *u_right,
                            float *depth_out);
/* The RGB-D Frame constructor for nframes host frames: extraction exactly as orbx_extract_batch (input format of
 * orbx_set_input_format, same chunks), then per frame kps_un / u_right / depth as orbx_rgbd_depth_device; depth frames have
 * the image's width and height.  Outputs [nframes][cap].  Depth reaches the device in one of two ways, with identical results:
 * uploaded chunk by chunk on the copy stream, or -- when `depth` is page-locked and device-mapped (orbx_host_alloc,
 * hipHostMalloc, hipHostRegister with the mapped flag) -- read in place by the kernel, one sample per keypoint.  The environment
 * variable ORBX_RGBD_DEPTH=upload|inplace (read per call) selects between them for mapped depth; the default is in DESIGN.md
 * section 0.  Like the output buffers of orbx_extract_batch, mapped kps_un / u_right / depth are written in place. */
orbx_status orbx_extract_rgbd_batch(orbx_handle *h, int nframes, const uint8_t *imgs, int width, int height, int stride,
                                    int64_t frame_stride, const void *depth, int depth_format, int depth_stride,
                                    int64_t depth_frame_stride, float depth_scale, const float *camera4, const float *dist,
                                    int ndist, float mbf, orbx_keypoint *kps, orbx_keypoint *kps_un, uint8_t *desc,
                                    int32_t *counts, float *u_right, float *depth_out, int cap);
/* Frame::AssignFeaturesToGrid + PosInGrid (src/Frame.cc:432-460, 729-745) on the device, for the keypoint buffers
 * orbx_extract_batch_device / orbx_undistort_keypoints_device filled (records `cap` apart, cap <= 65535): per frame
 * d_cell_begin[64 * 48 + 1] offsets (bucket c = column * 48 + row, the reference's mGrid[column][row]) into d_items[cap], the
 * feature indices of every bucket in ascending order (= push_back order).  bounds4 = mnMinX, mnMaxX, mnMinY, mnMaxY.
 * Asynchronous on the handle's stream: the keypoints do not leave the GPU between extraction and a gated match. */
orbx_status orbx_grid_build_device(orbx_handle *h, int nframes, const orbx_keypoint *d_kps, const int32_t *d_counts, int cap,
                                   const float *bounds4, int32_t *d_cell_begin, uint16_t *d_items);
/* The primitive behind every projection-guided policy: Frame::GetFeaturesInArea (src/Frame.cc:633-717, incl. the quirk
 * bCheckLevels = minLevel > 0 || maxLevel >= 0, :673) for nq queries against one target frame, fused with
 * ORBmatcher::DescriptorDistance.  Host buffers.  xyr = (x, y, r) per query (r < 0: no candidates), levels = (minLevel,
 * maxLevel) per query, qdesc = one descriptor per query.  begin[nq + 1] = offsets into items; items = the candidates of each
 * query in the reference's visiting order (column outer, row inner, bucket order), feature index | Hamming distance << 16.
 * *total = number of items (ORBX_CAPACITY if it exceeds items_cap; begin / total are valid then). */
orbx_status orbx_gated_candidates(orbx_handle *h, const orbx_keypoint *target_keys, const uint8_t *target_desc, int nt,
                                  const float *bounds4, const float *xyr, const int32_t *levels, const uint8_t *qdesc, int nq,
                                  uint32_t *begin, uint32_t *items, int items_cap, int *total);
/* mnMinX, mnMaxX, mnMinY, mnMaxY */
orbx_status orbx_image_bounds(orbx_handle *h, int cols, int rows, const float *camera4, const float *dist, int ndist,
                              float *bounds4);

/* Page-locked host memory for the host-buffer entry points: with it every upload / download of orbx_extract_batch is an
 * asynchronous DMA that overlaps the kernels of the neighbouring chunks (pageable memory works too, the runtime then
 * stages the copies and blocks the calling thread while it does).  A call with more frames than the handle's max_batch is
 * processed in chunks of max_batch frames, the upload of chunk c+1 overlapping the kernels of chunk c on ONE copy stream.
 * Keypoint / descriptor buffers allocated here (or any page-locked, device-mapped memory: hipHostMalloc, hipHostRegister
 * with the mapped flag) are not downloaded at all in such a call: the describe kernel writes its records straight into them
 * over the link, only the per-frame counts come back by copy; their contents are defined when the call returns, rows beyond
 * a frame's count are left as they were.  (640x480, 1000 features, chunks of 64: 134 k frames/s per 256-frame call, 155 k per
 * 1024-frame call from page-locked memory, 109-127 k from pageable memory.)  NULL on failure. */
void *orbx_host_alloc(size_t bytes);
void orbx_host_free(void *p);

/* ---- stream / timing plumbing ------------------------------------------------------------ */
void *orbx_get_stream(orbx_handle *h);            /* hipStream_t */
orbx_status orbx_set_stream(orbx_handle *h, void *hip_stream); /* NULL restores the private stream */
orbx_status orbx_synchronize(orbx_handle *h);
/* per-kernel HIP-event timing on the handle's stream.  mask bit k enables kernel id k. */
enum {
    ORBX_K_PYR_L0 = 0, ORBX_K_PYR_RESIZE = 1, ORBX_K_FAST = 2, ORBX_K_QUADTREE = 3, ORBX_K_ORIENT = 4,
    ORBX_K_BLUR = 5, ORBX_K_DESC = 6, ORBX_K_MATCH = 7, ORBX_K_MISC = 8, ORBX_K_COUNT = 9
};
orbx_status orbx_profile_enable(orbx_handle *h, uint32_t kernel_mask);
/* synchronises, then returns accumulated milliseconds and launch counts since the last reset */
orbx_status orbx_profile_read(orbx_handle *h, float *ms, int32_t *launches, int reset);
const char *orbx_kernel_name(int kernel_id);

/* ---- per-stage inspection of the last batch (parity tests only; synchronises) -------------- */
/* candidates of (frame, level) = vToDistributeKeys (src/ORBextractor.cc:1451-1548), border-relative
 * coordinates, in unspecified order; returns count via *n (may exceed cap => ORBX_CAPACITY) */
orbx_status orbx_debug_candidates(orbx_handle *h, int frame, int level, orbx_keypoint *out, int cap, int *n);
/* keypoints of (frame, level) after quadtree + orientation, level coordinates, list order */
orbx_status orbx_debug_level_keypoints(orbx_handle *h, int frame, int level, orbx_keypoint *out, int cap, int *n);
/* blurred level: GaussianBlur of mvImagePyramid[level] (fork: the padded level; upstream: the un-padded view) */
orbx_status orbx_debug_blur_copy(orbx_handle *h, int frame, int level, uint8_t *dst, int dst_stride);
/* FAST groups (waves' work items of k_fast_rows) per frame of the configured geometry: those of level 0, and all of them */
orbx_status orbx_debug_fast_groups(orbx_handle *h, int *level0, int *total);
/* The regime a launcher picks from the size of a launch alone, as it would on this handle (tests assert the regime they mean to
 * run in).  Pure arithmetic: no device work, host-only handles answer too.
 * orbx_debug_match_plan: orbx_match_bruteforce_device(npairs, ..., out_stride) with the handle's ORBX_MATCH_KERNEL -- qt = query
 * tiles of 32 per wave of the matrix-pipe kernels (4 or 2; 0 = the vector-pipe kernel), nsplit = blocks a pair's train set is
 * split over (1..16; 1 on the matrix pipe = direct output, no merge kernel).
 * orbx_debug_fast_gpw: groups per wave (1 or 2) of a k_fast_rows launch over `nframes` frames x `ngroups` groups -- the forced
 * value when ORBX_FAST_GPW=1|2 is set (read when the handle is configured; any other value is ORBX_BAD_ARGUMENT), else the size
 * rule. */
orbx_status orbx_debug_match_plan(orbx_handle *h, int npairs, int out_stride, int *qt, int *nsplit);
orbx_status orbx_debug_fast_gpw(orbx_handle *h, int nframes, int ngroups, int *gpw);
/* the two per-lane forms of the BRIEF pattern k_describe reads, as uploaded: 64 lanes x 16 coordinates (round r of lane l =
 * pair r*64 + l as x1, y1, x2, y2), int8 and float.  Host only: needs no handle and no device. */
orbx_status orbx_debug_describe_pattern(int8_t *lane_i8_1024, float *lane_f32_1024);

/* ---- Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:363-607), the reader of the tracking matchers' rows
 * (TrackWithMotionModel, TrackReferenceKeyFrame, TrackLocalMap, Relocalization), for many (frame, pose, matches) problems in
 * one call: one 6-DoF vertex, unary mono / stereo edges in feature order, four rounds of at most ten Levenberg-Marquardt
 * iterations of at most ten trials, inlier test after each round (k_pose_opt: one wave per problem).
 * CONTRACT: the device rows equal the library's host path (ORBX_POSE=host in the environment, read per call; host-only handles)
 * and the numpy restatement tests/pose_model.py bit for bit, in both fp_modes.  Parity with a g2o + Eigen build is NOT pinned:
 * DESIGN.md section 2 (F11) lists what follows the reference's source and every order of arithmetic this library fixes where
 * the reference leaves it to Eigen or libm (sums per edge and across edges, the 6x6 solve, powers, sin / cos).
 * The frames are read where the device batch left them (d_keys_un / d_u_right / d_counts as for the tracking matchers,
 * d_u_right == NULL: every edge monocular; mvuRight[i] < 0 is a monocular edge).  Row k of d_point ([nproblems][cap]) gives per
 * feature of problem k's frame -1 (no MapPoint) or the position of its MapPoint in the problem's list: a d_assigned row of
 * orbx_search_by_projection_mappoints_batch_device / orbx_search_local_points_batch_device is accepted as it stands (with the
 * same point_index); a d_matched_last row of orbx_search_by_projection_frame_batch_device maps the other way (last-frame point
 * -> current feature) and has to be inverted by the caller first.  The pool of world positions (host, 3 floats per point) is
 * uploaded once per call and shared by all problems; point_index == NULL: list position = pool index (npoints <= npool).
 * Results, on the device: d_Tcw row k = the optimised pose (Converter::toCvMat), d_outlier[k][i] = mvbOutlier[i] for every
 * feature i < min(count, cap) that has a MapPoint (other entries are not written), d_ninliers[k] = the return value.  Fewer
 * than 3 correspondences: d_ninliers[k] = 0, the d_Tcw row is NOT written (the reference returns before SetPose) and the outlier
 * entries of features with a MapPoint are 0, as the reference leaves them.  Asynchronous on the handle's stream, one
 * page-locked staging block consumed before the call returns, nothing downloaded.  Several problems may name one frame.
 * Validated before any device work: ORBX_BAD_ARGUMENT for nproblems < 0, a null array, a frame outside [0, nframes), cap <= 0,
 * npoints < 0, a point_index entry outside the pool; ORBX_UNSUPPORTED for cap > 65535.  The host cannot see device rows: a
 * d_point entry >= npoints or an octave outside [0, nlevels) makes the kernel treat that feature as one without a MapPoint (no
 * read leaves the pool or the level table); where the rows are host arrays (orbx_pose_optimization, host-only handles) both are
 * ORBX_BAD_ARGUMENT and nothing is written.  nproblems == 0 launches nothing.
 * On a host-only handle (device = -2) every "d_" argument is a HOST array and the host path runs.
 * OUTSIDE the contract: a point at z = 0 in the camera frame or non-finite input gives non-finite terms in the reference too.
 * The rule here: the same bounded loops run, a trial whose chi2 is not finite is never accepted (g2o_isfinite(tempChi)), a
 * 6x6 system with a pivot that is not positive and finite counts as a failed solve (chi2 = DBL_MAX, the step is rejected), and
 * a NaN chi2 in the inlier test compares as "not greater" (inlier), as the reference's float comparison does.  A point behind
 * the camera with finite terms is inside the contract. */
typedef struct orbx_pose_problem {
    int32_t frame;              /* this frame of the device batch */
    float   Tcw[16];            /* pFrame->mTcw on entry, row major */
    const int32_t *point_index; /* optional: list position -> pool index (as orbx_track_local_problem) */
    int32_t npoints;
} orbx_pose_problem;
orbx_status orbx_pose_optimization_batch_device(orbx_handle *h, int nproblems, const orbx_pose_problem *problems, int npool,
                                                const float *world_pos, int nframes, const orbx_keypoint *d_keys_un,
                                                const float *d_u_right, const int32_t *d_counts, int cap, const int32_t *d_point,
                                                const float *camera4, float mbf, const float *inv_level_sigma2, int nlevels,
                                                float *d_Tcw, uint8_t *d_outlier, int32_t *d_ninliers);
/* One frame, host arrays in and out, run on the library's host path (measured: one problem per call takes 0.24-3.3 ms on the
 * device against 53-586 us on the host path, profiles/pose_batch.md); works on a host-only handle.  point[i] = -1 or the pool index of feature i's MapPoint; Tcw is read
 * and, with at least 3 correspondences, overwritten; outlier[n]; *ninliers = the return value of the reference. */
orbx_status orbx_pose_optimization(orbx_handle *h, float *Tcw, int n, const orbx_keypoint *keys_un, const float *u_right,
                                   const int32_t *point, int npool, const float *world_pos, const float *camera4, float mbf,
                                   const float *inv_level_sigma2, int nlevels, uint8_t *outlier, int32_t *ninliers);
/* Parity tests only: the inlier test that ends a round (src/Optimizer.cc:534-592), alone, for the problems of a call shaped like
 * orbx_pose_optimization_batch_device.  Tcw_est / Tcw_last: host, [nproblems][16], the estimate and the pose at which
 * computeActiveErrors ran last (after a rejected trial the two differ, and the edges keep the rejected trial's errors).  Row k of
 * d_outlier holds the flags on entry (0 / 1 where a MapPoint exists): a flagged edge is tested at Tcw_est, every other edge at
 * Tcw_last; the new flags are written back and d_ninliers[k] = edges - flagged.  Device path, ORBX_POSE=host and host-only
 * handles as for the batch call. */
orbx_status orbx_debug_pose_inlier_test(orbx_handle *h, int nproblems, const orbx_pose_problem *problems, int npool,
                                        const float *world_pos, int nframes, const orbx_keypoint *d_keys_un, const float *d_u_right,
                                        const int32_t *d_counts, int cap, const int32_t *d_point, const float *camera4, float mbf,
                                        const float *inv_level_sigma2, int nlevels, const float *Tcw_est, const float *Tcw_last,
                                        uint8_t *d_outlier, int32_t *d_ninliers);
/* sin and cos as SE3Quat::exp gets them in both paths (csrc/orbx_pose.h: *, +, fma only; theta >= 0).  Exported for
 * tests/pose_model.py, which takes this one primitive from the library. */
void orbx_pose_sin_cos(double theta, double *s, double *c);

/* ---- Sim3Solver (src/Sim3Solver.cc), the RANSAC between SearchByBoW and OptimizeSim3 in LoopClosing::ComputeSim3
 * (src/LoopClosing.cc:487-577), for all candidates of the loop in one device round trip.  iterate() returns at iteration i iff
 * count_i >= max(count_j, j < i) and count_i > mRansacMinInliers (:267-286), so every iteration of every candidate is evaluated
 * ahead of time -- k_sim3_hypotheses: one lane per (problem, iteration) runs ComputeSim3 on the three drawn correspondences;
 * k_sim3_inliers: one wave per (problem, iteration) runs CheckInliers over the problem's correspondences staged in LDS, the
 * mask as 64-bit ballot words, the count as the sum of their popcounts -- and orbx_sim3_batch_iterate replays the reference's
 * iterate(n, ...) calls on the host from the stored counts, in any interleaving, including a solver that is iterated again
 * after its first answer was rejected.
 * CONTRACT: hypotheses, masks and counts of the device equal the library's host path (ORBX_SIM3=host in the environment, read
 * per call; host-only handles) and the numpy restatement tests/sim3_model.py bit for bit, in both fp_modes.  Parity with an
 * OpenCV build is NOT pinned from N to R: DESIGN.md section 2 (F12) lists what follows the reference's source and what this
 * library fixes where the reference leaves it to OpenCV (cv::eigen, cv::norm, the MatExpr scaling, cv::Rodrigues, the order of
 * the 3x3 float products, cv::Mat::dot) or to libm (atan2, sin, cos).
 * The caller supplies the draws: sets[i] = the three indices DUtils::Random::RandomInt gave iteration i, so a solver's answer
 * is the reference's for the same draws.  Repeated indices within a set are accepted (a degenerate hypothesis).
 * A problem with n < min_inliers launches nothing, its sets are not read (may be NULL) and its first iterate reports no_more.
 * Validated before any device work, ORBX_BAD_ARGUMENT: nproblems < 0, a null array whose size is positive, n < 0,
 * iterations < 1, a set index outside [0, n).  nproblems == 0 launches nothing and gives an empty batch.
 * OUTSIDE the contract (den == 0, a degenerate triple, z == 0 after a transform, non-finite input): the same straight-line
 * code runs, a non-finite err compares as "not less" and the point is an outlier. */
typedef struct orbx_sim3_problem {
    int32_t n;                        /* N of the solver: correspondences that passed the constructor's filters */
    const float *x1c, *x2c;           /* [n][3] mvX3Dc1, mvX3Dc2 */
    const float *max_err1, *max_err2; /* [n]   mvnMaxError1/2 */
    float camera1[4], camera2[4];     /* fx, fy, cx, cy of mK1, mK2 */
    int32_t fix_scale, min_inliers, iterations;   /* iterations = mRansacMaxIts AFTER SetRansacParameters */
    const int32_t *sets;              /* [iterations][3] indices into 0..n-1, the draws in order */
} orbx_sim3_problem;
typedef struct orbx_sim3_batch orbx_sim3_batch;
/* SetRansacParameters (:153-191) on the host: mRansacMaxIts for N = n (float epsilon, the host's log / pow, the
 * min_inliers == n branch, max(1, min(., .))) */
int32_t orbx_sim3_ransac_iterations(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations);
/* One page-locked block up, both kernels, one block down; the batch owns host copies of the results and needs neither the
 * handle nor the caller's arrays afterwards.  On a host-only handle the library's host path runs. */
orbx_status orbx_sim3_ransac_batch_create(orbx_handle *h, int nproblems, const orbx_sim3_problem *problems, orbx_sim3_batch **out);
/* Sim3Solver::iterate(n_iterations, bNoMore, vbInliers, nInliers) of solver k as a cursor over the stored results.  Returns 1
 * when a Sim3 is returned (T12 [16] row major = mBestT12, inliers [n] = mvbInliersi as 0 / 1, *ninliers), 0 when not (inliers
 * all 0, *ninliers = 0, T12 untouched), -1 for a bad argument (orbx_last_error()).  mnIterations, mnBestInliers and the best
 * hypothesis are kept per solver and updated on >= even when nothing is returned; *no_more follows :290. */
int32_t orbx_sim3_batch_iterate(orbx_sim3_batch *b, int k, int n_iterations, int32_t *no_more, uint8_t *inliers, int32_t *ninliers,
                                float *T12);
/* GetEstimatedRotation / Translation / Scale of solver k: R [9] row major, t [3], *s.  ORBX_BAD_ARGUMENT before the first
 * iteration of the solver has run (the reference returns empty matrices there). */
orbx_status orbx_sim3_batch_best(const orbx_sim3_batch *b, int k, float *R, float *t, float *s);
/* tests and tools: the inlier count of every iteration of solver k, counts [iterations] (nothing is written for a solver that
 * launched nothing); *niterations, optional, receives how many were written */
orbx_status orbx_sim3_batch_counts(const orbx_sim3_batch *b, int k, int32_t *counts, int32_t *niterations);
/* tests and tools: hypothesis `iteration` of solver k as 48 floats (T12 [16] | T21 [16] | R [9] | t [3] | s | 3 x 0) and its
 * mask words (uint64 [ceil(n / 64)], bit i of word w = correspondence 64 w + i); either pointer may be NULL */
orbx_status orbx_sim3_batch_hypothesis(const orbx_sim3_batch *b, int k, int iteration, float *hyp48, uint64_t *mask_words);
void orbx_sim3_batch_destroy(orbx_sim3_batch *b);
/* atan2(y, x) for y >= 0 as ComputeSim3 gets it in both paths (csrc/orbx_sim3.h: *, + and IEEE division only).  Exported for
 * tests/sim3_model.py, which takes this primitive and orbx_pose_sin_cos from the library. */
double orbx_sim3_atan2(double y, double x);

/* ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:1383-1615), the link after SearchBySim3 in LoopClosing::ComputeSim3, for every
 * candidate that returned a Sim3 in one round (and for many streams) in one call.  All VertexSBAPointXYZ are fixed, so the
 * system is ONE dense 7x7 around a VertexSim3Expmap; g2o takes the Jacobians of EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ
 * numerically (central differences, delta = 1e-9), so an edge costs 1 + 14 map-and-project evaluations under 14 perturbed
 * Sim3 that are the same for every edge.  optimize(5), the chi2 test, return 0 below 10 survivors, optimize(5 or 10), the
 * chi2 test (k_sim3_opt: one wave per problem, one problem per workgroup).
 * CONTRACT: results and keep rows of the device equal the library's host path (ORBX_SIM3OPT=host in the environment, read per
 * call; host-only handles) and the numpy restatement tests/sim3opt_model.py bit for bit, in both fp_modes.  Parity with a g2o +
 * Eigen build is NOT pinned: DESIGN.md section 2 (F16) lists what follows the reference's source and what this library fixes
 * where the reference leaves it to Eigen (product and summation orders, the dense solve) or to libm (exp, sin, cos).
 * The caller runs the pointer-chasing filters (pMP1 && pMP2, isBad, GetIndexInKeyFrame >= 0) and the float products
 * R1w * P3D1w + t1w; a problem lists the correspondences that passed, in order of i.
 * Results: keep[i] = 1 where vpMatches1[idx_i] survives, 0 where the reference nulls it (the first test's nulls are present
 * also when the call then returns 0); written = 1 iff the reference assigns g2oS12, r / t / s are then the optimised Sim3,
 * otherwise the input as g2o::Sim3(R, t, s) holds it; ninliers is the return value; nbad the first test's count.
 * Validated before any device work, ORBX_BAD_ARGUMENT: nproblems < 0, a null array whose size is positive, n < 0.
 * nproblems == 0 launches nothing.  n == 0 gives ninliers = 0, written = 0 and reads no array of the problem.
 * OUTSIDE the contract (z == 0 after a map, s == 0, non-finite input): the same straight-line code runs, every loop is
 * bounded, a NaN chi2 compares as "not greater" (an inlier, as in the reference) and every stored NaN is the canonical one.
 * MEASURED on an MI355X (tools/sim3opt_rate.py, profiles/sim3opt_batch.md; n = 30 / 100 / 300 correspondences, against the
 * library's own host path on one core, which is neither g2o nor the reference): ONE problem per call loses on the device,
 * 188 / 357 / 776 us against 36 / 91 / 263 us; 16 per call 14 / 26 / 57 us each against 32 / 94 / 279 us; 256 per call
 * 1.0 / 2.0 / 4.7 us each.  A caller with one candidate at a time uses a host-only handle (compat/Optimizer_sim3.inl does). */
typedef struct orbx_sim3opt_problem {
    int32_t n;                         /* correspondences that passed OptimizeSim3's own filters, in order of i */
    const float *x1c, *x2c;            /* [n][3] P3D1c, P3D2c */
    const float *obs1, *obs2;          /* [n][2] kpUn1.pt, kpUn2.pt */
    const float *inv_sigma2_1, *inv_sigma2_2;   /* [n] */
    float camera1[4], camera2[4];      /* fx, fy, cx, cy */
    float R[9], t[3], s;               /* the solver's estimate (orbx_sim3_batch_best) */
    float th2; int32_t fix_scale;
    uint8_t *keep;                     /* [n] out: 1 = vpMatches1[idx] survives */
} orbx_sim3opt_problem;
typedef struct orbx_sim3opt_result {
    double r[4], t[3], s;              /* g2oS12 on return: quaternion x, y, z, w; the input when written == 0 */
    float T12[16];                     /* Converter::toCvMat(g2oS12): [sR | t] */
    int32_t ninliers, nbad, ncorr, written;
} orbx_sim3opt_result;
/* One page-locked block up, k_sim3_opt, one block down, the wait.  On a host-only handle the library's host path runs. */
orbx_status orbx_optimize_sim3_batch(orbx_handle *h, int nproblems, const orbx_sim3opt_problem *problems, orbx_sim3opt_result *results);
/* parity tests only: the chi2 test alone on all n correspondences of each problem, with the Sim3 at which computeActiveErrors
 * ran last given explicitly (S_last [nproblems][8]: r x y z w, t, s); keep as after the first test, nbad = its count,
 * ninliers = n - nbad, written = 0, r / t / s = the input.  Device path, ORBX_SIM3OPT=host and host-only handles. */
orbx_status orbx_debug_sim3opt_inlier_test(orbx_handle *h, int nproblems, const orbx_sim3opt_problem *problems, const double *S_last,
                                           orbx_sim3opt_result *results);
/* exp as Sim3(Vector7d) gets it in both paths (csrc/orbx_sim3opt.h: *, +, fma only).  Exported for tests/sim3opt_model.py,
 * which takes this primitive and orbx_pose_sin_cos from the library. */
double orbx_sim3opt_exp(double sigma);

/* ---- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:631-1030), the last heavy stage of LocalMapping::Run, from the point
 * where the reference holds lLocalKeyFrames, lFixedCameras and lLocalMapPoints with their observations (:710) to the optimised
 * poses, the optimised points and vToErase (:991), for many problems in one call.  Every edge joins one keyframe and one
 * point and all points are marginalised, so H_pp is 6x6 block diagonal, H_ll 3x3 block diagonal, and the only coupled system is
 * the Schur complement over the free keyframes: dense, 6 per free keyframe wide (k_local_ba: one workgroup per problem).
 * optimize(5) with Huber on every edge, the classification (chi2 > 5.991 / 7.815 || !isDepthPositive; flagged edges leave the
 * system, the kernel comes off every edge), optimize(10) when second_round, the final classification into erase.
 * A problem is flat host arrays.  Keyframes: the nlocal local ones in list order, then the nfixed fixed ones; local_fixed[k]
 * carries mnId == 0 (:738).  camera (fx, fy, cx, cy) and bf are per problem.  Observations are CSR by point (obs_begin); within a
 * point the caller's order stands (the reference walks a std::map<KeyFrame*, size_t>: pointer order); obs = kpUn.pt.x, kpUn.pt.y,
 * mvuRight (< 0: a monocular edge); bad keyframes are left out by the caller (:813).  second_round is what bDoMore would be: the
 * reference samples *pbStopFlag between the rounds, a batch call cannot, so the caller decides before the call (and does not
 * call at all with the flag set on entry, :886-888).  The library classifies every edge: pMP->isBad() inside the two
 * classification loops cannot be seen from a snapshot; the caller drops an erase entry whose point has gone bad.
 * Results: Tcw_out[k] = Converter::toCvMat(vSE3->estimate()) for EVERY local keyframe (a locally fixed one gets the quaternion
 * round trip of its input, as SetPose does in the reference); world_out; erase[e] = 1 where the pair goes into vToErase.
 * CONTRACT: the device equals the library's host path (ORBX_LOCALBA=host in the environment, read per call; host-only handles)
 * and the numpy restatement tests/localba_model.py bit for bit, in both fp_modes.  Parity with a g2o + Eigen build is NOT
 * pinned: DESIGN.md section 2 (F19) lists what follows the reference's source and what this library fixes where the reference
 * leaves it to Eigen and to a sparse Cholesky with a fill-reducing ordering.
 * Validated before any device work, ORBX_BAD_ARGUMENT: nproblems < 0, a null array whose size is positive, a negative count, an
 * obs_begin that does not start at 0 or decreases, an obs_kf outside the keyframe list, a point that lists one keyframe twice;
 * ORBX_UNSUPPORTED: nlocal > 128 (the reduced system's workspace), more than 4000000 observations in a problem.  Outputs of a
 * rejected call are not written.  nproblems == 0 launches nothing.
 * OUTSIDE the contract (z == 0 in a keyframe, non-finite input, a keyframe without edges): the same bounded loops run
 * ((5 + 10) iterations x 10 trials), a failed reduced solve gives chi2 = DBL_MAX, and every stored NaN is the canonical one.
 * MEASURED: profiles/localba_batch.md. */
typedef struct orbx_localba_problem {
    int32_t nlocal, nfixed, npoints;
    int32_t second_round;              /* 0 / 1: what bDoMore would be */
    const float *Tcw;                  /* [nlocal + nfixed][16] */
    const uint8_t *local_fixed;        /* [nlocal] mnId == 0 */
    float camera[4], bf;
    const float *world;                /* [npoints][3] */
    const int32_t *obs_begin;          /* [npoints + 1] */
    const int32_t *obs_kf;             /* [nobs] index into the keyframe list */
    const float *obs;                  /* [nobs][3] */
    const float *inv_sigma2;           /* [nobs] */
    float *Tcw_out;                    /* [nlocal][16] out */
    float *world_out;                  /* [npoints][3] out */
    uint8_t *erase;                    /* [nobs] out */
} orbx_localba_problem;
typedef struct orbx_localba_result {
    int32_t iters[2];                  /* iterations run by optimize(5), optimize(10) */
    int32_t nflagged, nerase;          /* edges at level 1 after the first classification; entries of vToErase */
    double chi2[4];                    /* activeRobustChi2 at the first linearisation and at the end of round 1, of round 2 */
} orbx_localba_result;
/* One page-locked block up, k_local_ba, one block down, the wait.  Synchronous: the results go straight back into the map. */
orbx_status orbx_local_bundle_adjustment_batch(orbx_handle *h, int nproblems, const orbx_localba_problem *problems,
                                               orbx_localba_result *results);
/* parity tests only: the classification alone on every edge, chi2 at the estimates where computeActiveErrors ran last
 * (Tcw_last, world_last) and isDepthPositive at the current estimates (Tcw_est, world_est); arrays as in the problem.  Writes
 * erase and nerase; Tcw_out and world_out are not written. */
typedef struct orbx_localba_debug {
    const float *Tcw_est, *world_est, *Tcw_last, *world_last;
} orbx_localba_debug;
orbx_status orbx_debug_localba_classify(orbx_handle *h, int nproblems, const orbx_localba_problem *problems,
                                        const orbx_localba_debug *states, orbx_localba_result *results);

/* ---- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1050-1358), the pose graph over all keyframes that
 * LoopClosing::CorrectLoop runs after SearchAndFuse, for many problems in one call.  Every vertex is a VertexSim3Expmap, nothing is
 * marginalised, every edge is an EdgeSim3 with identity information and no robust kernel, and g2o takes its Jacobians
 * numerically (central differences, delta = 1e-9).  The normal equations are 7 x 7 block-sparse over the free keyframes; the
 * library factors them by a block L D L^T in an elimination order it fixes itself (rounds of independent low-degree vertices,
 * k_essential_graph: one workgroup per problem), runs Levenberg-Marquardt with setUserLambdaInit(1e-16) for at most 20
 * iterations, recovers Tiw = [R, t / s] (:1304-1321) and maps every map point through Srw and correctedSwr (:1326-1357,
 * k_eg_correct_points: one lane per point).
 * A problem is flat host arrays.  Vertices: Scw[v] = vScw (CorrectedSim3 where the keyframe has one, else (Rcw, tcw, 1)) as the
 * quaternion x y z w, t and s, 8 doubles; fixed[v] (pKF == pLoopKF); optionally non_corrected[v] with has_non_corrected[v]
 * (NonCorrectedSim3).  Only keyframes that are not bad are passed (the reference dereferences optimizer.vertex(id) of a bad one
 * at :1166 and :1308).  Edges: (i, j, kind) with vertex 0 = i and vertex 1 = j of the EdgeSim3; kind 1 is a loop-connection edge
 * of step 3, whose measurement Sji = Sjw * Swi takes both poses from Scw; kind 0 is an edge of step 4 (spanning tree, loop
 * edge, covisibility), which prefers non_corrected where present.  The library computes the measurements.  Parallel edges on
 * one pair are allowed, as in the reference.  A fixed vertex, or a vertex without an edge, leaves the system; an edge between
 * two fixed vertices is not active.  Points: world[p] and ref[p], the index of the vertex the point is corrected by
 * (mnCorrectedReference or the reference keyframe), -1 for a bad point, which is copied through.
 * Results: Siw_out[v] = the corrected Siw, 8 doubles; Tiw_out[v] = [R, t / s] narrowed to float, for EVERY vertex (a vertex
 * outside the system gets the round trip of its input); world_out; the record below.
 * CONTRACT: the device equals the library's host path (ORBX_ESSGRAPH=host in the environment, read per call; host-only handles)
 * and the numpy restatement tests/essgraph_model.py bit for bit, in both fp_modes.  Parity with a g2o + Eigen build is NOT
 * pinned: DESIGN.md section 2 (F20) lists what follows the reference's source and what this library fixes where the reference
 * leaves it to libm, to Eigen and to a sparse Cholesky with a fill-reducing ordering.
 * Validated before any device work, ORBX_BAD_ARGUMENT: nproblems < 0, a null array whose size is positive, a negative count, an
 * edge index outside the vertices, i == j, a kind other than 0 / 1, a non-finite pose, s <= 0, a ref outside [-1, nvertices);
 * ORBX_UNSUPPORTED: more than 2^20 vertices or 2^22 edges in a problem; ORBX_CAPACITY: on the device path, a problem whose L has
 * more than ORBX_ESSGRAPH_MAX_LBLOCKS blocks (the host path has no such cap).  Outputs of a rejected call are not written.
 * nproblems == 0 launches nothing.
 * OUTSIDE the contract (estimates that leave s > 0, a component without a fixed vertex): the same bounded loops run (20
 * iterations x 10 trials), a failed factorisation gives x = 0 and chi2 = DBL_MAX, and every stored NaN is the canonical one.
 * MEASURED: profiles/essgraph_batch.md. */
#define ORBX_ESSGRAPH_MAX_LBLOCKS 32768
typedef struct orbx_essgraph_problem {
    int32_t nvertices, nedges, npoints;
    int32_t fix_scale;                 /* 0 / 1: bFixScale */
    const double *Scw;                 /* [nvertices][8] */
    const uint8_t *fixed;              /* [nvertices] */
    const double *non_corrected;       /* [nvertices][8], or NULL: none */
    const uint8_t *has_non_corrected;  /* [nvertices], or NULL: none */
    const int32_t *edges;              /* [nedges][3] i, j, kind */
    const float *world;                /* [npoints][3] */
    const int32_t *ref;                /* [npoints] */
    double *Siw_out;                   /* [nvertices][8] out */
    float *Tiw_out;                    /* [nvertices][16] out */
    float *world_out;                  /* [npoints][3] out */
} orbx_essgraph_problem;
typedef struct orbx_essgraph_result {
    int32_t iters;                     /* iterations run by optimize(20) */
    int32_t nactive;                   /* vertices in the system */
    int32_t nfailed;                   /* solves whose factorisation was not positive */
    int32_t nrounds, nlblocks;         /* elimination rounds; 7 x 7 blocks of L, the diagonal ones included */
    int32_t pad;
    double chi2[2];                    /* activeChi2 at the first linearisation and at the end */
    double lambda;                     /* at the end */
} orbx_essgraph_result;
/* One page-locked block up, k_essential_graph and k_eg_correct_points, one block down, the wait.  Synchronous. */
orbx_status orbx_optimize_essential_graph_batch(orbx_handle *h, int nproblems, const orbx_essgraph_problem *problems,
                                                orbx_essgraph_result *results);
/* tests and tools: the library's log (Sim3::log's std::log), x > 0; and Sim3::log of (r x y z w, t, s) into out[7] */
double orbx_essgraph_log(double x);
void orbx_essgraph_sim3_log(const double *S8, double *out7);
/* g2o::Sim3(toMatrix3d(Rcw), toVector3d(tcw), 1.0) (:1109-1111) of a keyframe pose Tcw [16] as the 8 doubles of an Scw row: the
 * floats widened, Eigen's Quaterniond(Matrix3d), nothing normalised */
void orbx_essgraph_sim3_from_tcw(const float *Tcw, double *S8);

/* ---- PnPsolver (src/PnPsolver.cc), the EPnP RANSAC between SearchByBoW and PoseOptimization in Tracking::Relocalization
 * (src/Tracking.cc:2336-2366), for all candidate keyframes in one device round trip.  An iteration is an independent 4-point
 * EPnP followed by one projection of every correspondence, so every iteration of every candidate is evaluated ahead of time --
 * k_pnp_hypotheses: one lane per (problem, iteration) runs compute_pose on the four drawn correspondences in a lane-interleaved
 * LDS workspace; k_pnp_inliers: one wave per (problem, iteration) runs CheckInliers over the problem's correspondences staged in
 * LDS, the mask as 64-bit ballot words, the count as the sum of their popcounts -- and orbx_pnp_batch_iterate replays the
 * reference's iterate(n, ...) calls on the host from the stored counts and masks, in any interleaving: the OR loop condition
 * (:285), the strict > best update, Refine() after every qualifying iteration (on the host, cached per best mask), the
 * fall-through return of mBestTcw.
 * CONTRACT: hypotheses (double R and t, float Tcw, the chosen N), masks and counts of the device equal the library's host path
 * (ORBX_PNP=host in the environment, read per call; host-only handles) and the numpy restatement tests/pnp_model.py bit for bit,
 * in both fp_modes.  Parity with an OpenCV build is NOT pinned: DESIGN.md section 2 (F13) lists what follows the reference's
 * source and what this library fixes where the reference leaves it to OpenCV 1.x (cvSVD, cvInvert, cvSolve, cvMulTransposed).
 * The caller supplies the draws: sets[i] = the four indices the swap-remove draw of iteration i produced, so a solver's answer
 * is the reference's for the same draws.
 * A problem with n < min_inliers launches nothing, its sets are not read (may be NULL) and its first iterate reports no_more.
 * Validated before any device work, ORBX_BAD_ARGUMENT: nproblems < 0, a null array whose size is positive, n < 0,
 * iterations < 1, a set index outside [0, n), an index repeated within its set (the reference's draw cannot repeat).
 * nproblems == 0 launches nothing and gives an empty batch.
 * OUTSIDE the contract (a negative eigenvalue under sqrt, the singular branch of qr_solve, betas[0] == 0, z == 0, non-finite
 * input): the same straight-line code runs, qr_solve's singular branch gives X = 0, a non-finite error2 is an outlier, a stored
 * NaN is the canonical quiet NaN. */
typedef struct orbx_pnp_problem {
    int32_t n;                 /* N of the solver: correspondences that passed the constructor's filters */
    const float *p3dw;         /* [n][3] mvP3Dw */
    const float *p2d;          /* [n][2] mvP2D */
    const float *max_err;      /* [n]    mvMaxError = mvSigma2 * th2 (float times float) */
    double camera[4];          /* fu, fv, uc, vc */
    int32_t min_inliers, iterations;   /* mRansacMinInliers, mRansacMaxIts AFTER SetRansacParameters */
    const int32_t *sets;       /* [iterations][4] indices into 0..n-1, the draws in order */
} orbx_pnp_problem;
typedef struct orbx_pnp_batch orbx_pnp_batch;
/* SetRansacParameters (:190-239) on the host: mRansacMinInliers and mRansacMaxIts for N = n (N * epsilon truncated, float
 * epsilon, exponent 3, the min_inliers == N branch, max(1, min(., .))).  A double outside int's range converts as in
 * orbx_sim3_ransac_iterations.  Either result pointer may be NULL. */
void orbx_pnp_ransac_parameters(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations, int32_t min_set,
                                float epsilon, int32_t *out_min_inliers, int32_t *out_iterations);
/* One page-locked block up, both kernels, one block down; the batch owns copies of the problems and of the results and needs
 * neither the handle nor the caller's arrays afterwards.  On a host-only handle the library's host path runs. */
orbx_status orbx_pnp_ransac_batch_create(orbx_handle *h, int nproblems, const orbx_pnp_problem *problems, orbx_pnp_batch **out);
/* PnPsolver::iterate(n_iterations, bNoMore, vbInliers, nInliers) of solver k as a cursor over the stored results.  Returns 1
 * when a pose is returned (Tcw [16] row major = mRefinedTcw or mBestTcw, inliers [n] as 0 / 1, *ninliers), 0 when not (inliers
 * all 0, *ninliers = 0, Tcw untouched), -1 for a bad argument (orbx_last_error()), and -2 WITH THE SOLVER'S STATE UNCHANGED when
 * the replay would need an iteration past those stored: append sets and call again. */
int32_t orbx_pnp_batch_iterate(orbx_pnp_batch *b, int k, int n_iterations, int32_t *no_more, uint8_t *inliers, int32_t *ninliers,
                               float *Tcw);
/* Evaluates nsets further iterations of solver k (sets [nsets][4]) on the library's host path -- the same header code, the same
 * bits -- and appends them to its stored results, so any call pattern is the reference's, including a solver iterated again
 * past mRansacMaxIts after PoseOptimization rejected its answer. */
orbx_status orbx_pnp_batch_append(orbx_pnp_batch *b, int k, int nsets, const int32_t *sets);
/* tests and tools: mBestTcw [16], mnBestInliers and the iteration behind them (any pointer may be NULL); ORBX_BAD_ARGUMENT
 * before an iteration of the solver has reached min_inliers */
orbx_status orbx_pnp_batch_best(const orbx_pnp_batch *b, int k, float *Tcw, int32_t *ninliers, int32_t *iteration);
/* tests and tools: the inlier count of every stored iteration of solver k (counts may be NULL to ask for *niterations only) */
orbx_status orbx_pnp_batch_counts(const orbx_pnp_batch *b, int k, int32_t *counts, int32_t *niterations);
/* tests and tools: stored iteration `iteration` of solver k: Rt12 = double R [9] | t [3], Tcw float [16], *N the chosen
 * candidate, mask words (uint64 [ceil(n / 64)], bit i of word w = correspondence 64 w + i); any pointer may be NULL */
orbx_status orbx_pnp_batch_hypothesis(const orbx_pnp_batch *b, int k, int iteration, double *Rt12, float *Tcw, int32_t *N,
                                      uint64_t *mask_words);
void orbx_pnp_batch_destroy(orbx_pnp_batch *b);

/* ---- Initializer (src/Initializer.cc), the H / F RANSAC of monocular initialisation: what Initializer::Initialize runs on its
 * two threads (:204-215) between SearchForInitialization and ReconstructH / ReconstructF (which follow below:
 * orbx_init_reconstruct_batch_create, and both in one round trip: orbx_initialize_batch_create), for any number of initialisation
 * attempts in one device round trip.  An iteration is an independent eight-point DLT followed by one pass over every match, so
 * every iteration of both models of every attempt is evaluated at once -- k_init_hypotheses: one lane per (problem, model,
 * iteration) builds A from the eight normalised matches, takes its null vector in a lane-interleaved LDS workspace, projects F
 * to rank 2, de-normalises and inverts H; k_init_scores: one lane per hypothesis runs CheckHomography / CheckFundamental over
 * the problem's matches staged in LDS, the score as the float sum in match order, the mask as 64-bit words -- and the best
 * iteration per model, the first strict maximum of the score from 0, is picked on the host after the one download.
 * CONTRACT: Normalize's T1 and T2, hypotheses (the 3 x 3 matrix, for H its inverse), scores, masks, best iterations, RH and the
 * model of the device equal the library's host path (ORBX_INIT=host in the environment, read per call; host-only handles) and
 * the numpy restatement tests/init_model.py bit for bit, in both fp_modes.  Parity with an OpenCV build is NOT pinned:
 * DESIGN.md section 2 (F14) lists what follows the reference's source and what this library fixes where the reference leaves
 * it to OpenCV (cv::SVDecomp, cv::Mat::inv, the matrix products).
 * Normalize runs over ALL keypoints of each frame (keys1, keys2), as in the source, not over the matched ones.  The caller
 * supplies the draws: sets[i] = mvSets[i], so an attempt's answer is the reference's for the same draws.
 * model is ORBX_INIT_H iff RH = SH / (SH + SF) > 0.40, else ORBX_INIT_F, and ORBX_INIT_NONE when no iteration of either
 * requested model scored above 0 (the reference would then read an empty cv::Mat): SH = SF = 0, itH = itF = -1, H21 and F21
 * zero, masks all false, RH the canonical NaN.  A model that was not requested has score 0, iteration -1 and an all-false mask.
 * A problem with n < 8 launches nothing, its sets are not read (may be NULL) and it reports ORBX_INIT_NONE.
 * Validated before any device work, ORBX_BAD_ARGUMENT: nproblems < 0, a negative count, a null array whose size is positive,
 * iterations < 1, sigma not finite or not > 0, a bit of models outside H | F, a match index outside its frame, a set index outside
 * [0, n), an index repeated within its set (the reference's draw cannot repeat).  nproblems == 0 gives an empty batch.
 * OUTSIDE the contract (collinear or repeated points in a set, non-finite keypoints): the same straight-line code runs, a NaN
 * chi-square is added to the score and leaves bIn alone as in the source, a NaN score never wins (strict >), a stored NaN is
 * the canonical quiet NaN. */
#define ORBX_INIT_NONE 0
#define ORBX_INIT_H 1
#define ORBX_INIT_F 2
typedef struct orbx_init_problem {
    int32_t n1, n2;  const float *keys1, *keys2;   /* [n1][2], [n2][2]: mvKeys1 / mvKeys2 pt of ALL keypoints */
    int32_t n;       const int32_t *matches;        /* [n][2] mvMatches12 in order (index in 1, index in 2) */
    float sigma;     int32_t iterations;            /* mSigma, mMaxIterations */
    const int32_t *sets;                            /* [iterations][8] mvSets: the caller's draws, indices into 0..n-1 */
    int32_t models;                                 /* ORBX_INIT_H | ORBX_INIT_F */
} orbx_init_problem;
typedef struct orbx_init_batch orbx_init_batch;
/* One page-locked block up, both kernels, one block down; the batch owns copies of the results and needs neither the handle
 * nor the caller's arrays afterwards.  On a host-only handle the library's host path runs. */
orbx_status orbx_init_ransac_batch_create(orbx_handle *h, int nproblems, const orbx_init_problem *problems, orbx_init_batch **out);
/* What FindHomography and FindFundamental leave behind for problem k, and Initialize's choice: SH, SF, H21 [9], F21 [9] (row
 * major), the best masks as 0 / 1 per match [n], the iterations behind them (-1: none), RH, model.  Any pointer may be NULL. */
orbx_status orbx_init_batch_result(const orbx_init_batch *b, int k, float *SH, float *SF, float *H21, float *F21,
                                   uint8_t *inliersH, uint8_t *inliersF, int32_t *itH, int32_t *itF, float *RH, int32_t *model);
/* tests and tools: currentScore of every iteration of one model (scores may be NULL to ask for *niterations only; 0 iterations
 * for a model that was not requested or a problem that launched nothing) */
orbx_status orbx_init_batch_scores(const orbx_init_batch *b, int k, int model, float *scores, int32_t *niterations);
/* tests and tools: one iteration of one model: H21i or F21i [9], H12i [9] (zeros for F), its score, its mask words (uint64
 * [ceil(n / 64)], bit i of word w = match 64 w + i); any pointer may be NULL */
orbx_status orbx_init_batch_hypothesis(const orbx_init_batch *b, int k, int model, int iteration, float *M9, float *Minv9,
                                       float *score, uint64_t *mask_words);
/* tests and tools: Normalize's T1 and T2 [9] each, row major */
orbx_status orbx_init_batch_normalization(const orbx_init_batch *b, int k, float *T1, float *T2);
void orbx_init_batch_destroy(orbx_init_batch *b);

/* ---- Initializer, from the winning matrix to a map: ReconstructF (:963-1132) or ReconstructH (:1154-1462) with DecomposeE,
 * CheckRT and Triangulate, for any number of attempts in one device round trip.  Any matrix and inlier mask go in (the result of
 * orbx_init_batch_result, or anything else); R21, t21, the triangulated points and their flags come out.
 * k_init_decompose: one lane per problem forms E21 = (K^T F21) K or A = (Kinv H21) K, takes the 3 x 3 SVD and stores the 4 (F) or
 * 8 (H) pose hypotheses with P2 = K [R | t] and O2 = -R^T t.  k_init_check_rt: one wave per (problem, pose hypothesis), the
 * lanes striding over the matches; per inlier match Triangulate (the 4 x 4 null vector in registers) and the tests of CheckRT,
 * nGood as a ballot count, vCosParallax[min(50, size - 1)] as an exact selection by value (32 bisection steps on the integer key
 * of the float: no sort, no atomics).  k_init_pick: one wave per problem copies the planes of the only hypothesis that can win
 * -- F: the first i with nGood_i == maxGood; H: the first strict maximum -- into the block that is downloaded.  acos and the
 * accept / reject arithmetic of both functions run on the host in double, once per hypothesis.
 * CONTRACT: every R, t, n, nGood, cosine, parallax, status byte, point, the chosen hypothesis and ok of the device equal the
 * library's host path (ORBX_RECON=host in the environment, read per call; host-only handles) and the numpy restatement
 * tests/recon_model.py bit for bit, in both fp_modes.  Parity with an OpenCV build is NOT pinned: DESIGN.md section 2 (F15)
 * lists what follows the reference's source and what this library fixes where the reference leaves it to OpenCV or libm (the
 * 3 x 3 and 4 x 4 SVD, cv::determinant, cv::norm, Mat::dot, the products, Mat / scalar, the order statistic, acosf).
 * Outputs are per MATCH, in match order, not per keypoint: status 0 -- skipped or rejected, 1 -- the point is not finite
 * (vbGood[first] = false), 2 -- counted in nGood (the point is stored), 3 -- counted and vbGood[first] = true.  Scattering them
 * to vP3D[first] / vbTriangulated[first] in match order reproduces the reference for repeated `first` indices too.
 * A problem with n == 0 or an all-false mask launches nothing and reports failure with zero counts.
 * Validated before any device work, ORBX_BAD_ARGUMENT: nproblems < 0, a negative count, a null array whose size is positive, a
 * model that is neither ORBX_INIT_H nor ORBX_INIT_F, a match index outside its frame, sigma or an intrinsic that is not finite,
 * sigma, fx or fy not > 0, min_parallax NaN.  nproblems == 0 gives an empty batch.
 * OUTSIDE the contract (dist1 * dist2 == 0, non-finite keypoints or matrix): the same straight-line code runs, a NaN compares
 * false wherever the source compares it, a stored NaN is the canonical quiet NaN and sorts after +infinity. */
typedef struct orbx_recon_problem {
    int32_t n1, n2;  const float *keys1, *keys2;   /* [n1][2], [n2][2]: mvKeys1 / mvKeys2 pt */
    int32_t n;       const int32_t *matches;        /* [n][2] mvMatches12 in order (index in 1, index in 2) */
    const uint8_t *inliers;                         /* [n] vbMatchesInliers, 0 = false */
    int32_t model;                                  /* ORBX_INIT_H: M is H21 (ReconstructH); ORBX_INIT_F: M is F21 (ReconstructF) */
    float M[9];                                     /* row major */
    float K[4];                                     /* fx, fy, cx, cy */
    float sigma;                                    /* mSigma */
    float min_parallax;                             /* minParallax, 1.0 in Initialize */
    int32_t min_triangulated;                       /* minTriangulated, 50 in Initialize */
} orbx_recon_problem;
typedef struct orbx_recon_batch orbx_recon_batch;
/* One page-locked block up, three kernels, one block down; the batch owns copies of the results and needs neither the handle
 * nor the caller's arrays afterwards.  On a host-only handle the library's host path runs. */
orbx_status orbx_init_reconstruct_batch_create(orbx_handle *h, int nproblems, const orbx_recon_problem *problems,
                                               orbx_recon_batch **out);
/* Problem k: ok (the function's return value), R21 [9] and t21 [3] (zeros when not ok, where the reference leaves empty
 * cv::Mat), the hypothesis the points belong to (-1: none -- nothing launched, ReconstructH returned early, or every count of
 * ReconstructH was 0), its per-match status [n] and points [n][3] (zeros where nothing was stored; they are filled whether ok or
 * not, the reference copies them only when ok), and N, the number of true mask entries.  Any pointer may be NULL. */
orbx_status orbx_recon_batch_result(const orbx_recon_batch *b, int k, int32_t *ok, float *R21, float *t21, int32_t *chosen,
                                    uint8_t *status, float *points, int32_t *N);
/* tests and tools: pose hypothesis i of problem k (0..3 for F, 0..7 for H): R [9], t [3], n [3] (zeros for F), nGood, the
 * selected cosine (0 when nGood == 0), parallax in degrees, valid (0: not evaluated); any pointer may be NULL */
orbx_status orbx_recon_batch_hypothesis(const orbx_recon_batch *b, int k, int i, float *R9, float *t3, float *n3, int32_t *nGood,
                                        float *cosine, float *parallax, int32_t *valid);
void orbx_recon_batch_destroy(orbx_recon_batch *b);
/* Initializer::Initialize from :204 to its return, for any number of attempts in ONE upload and ONE download: hypotheses, scores,
 * k_init_select (one wave per problem: the first strict maximum of each model's scores from 0, RH and the model by the rule and
 * with the bits of orbx_init_ransac_batch_create; it writes the winning matrix, the model and the winning mask as inlier bytes
 * where the reconstruction kernels read them), decompose, check, pick.  cameras[k] goes with problems[k].
 * CONTRACT: *ransac equals what orbx_init_ransac_batch_create gives for the same problems and *recon what
 * orbx_init_reconstruct_batch_create gives when fed with that result (the chosen model's matrix and mask), bit for bit.  A problem
 * whose model is ORBX_INIT_NONE reconstructs nothing and reports failure; it reads as an F problem with an all-false mask.
 * The fused sequence runs on a device handle when neither ORBX_INIT nor ORBX_RECON is "host"; otherwise the two calls run one after
 * the other, each by its own switch.  Validation is that of both calls, before any device work. */
typedef struct orbx_init_camera {
    float K[4];                                     /* fx, fy, cx, cy */
    float min_parallax;                             /* 1.0 in Initialize */
    int32_t min_triangulated;                       /* 50 in Initialize */
} orbx_init_camera;
orbx_status orbx_initialize_batch_create(orbx_handle *h, int nproblems, const orbx_init_problem *problems,
                                         const orbx_init_camera *cameras, orbx_init_batch **ransac, orbx_recon_batch **recon);

/* ---- LocalMapping::CreateNewMapPoints, the per-match geometry of src/LocalMapping.cc:450-651 between SearchForTriangulation
 * (orbx_triangulation_batch_*) and the refresh of the new points (orbx_distinctive_descriptors_batch,
 * orbx_update_normal_and_depth_batch): the ray-parallax test, the choice between linear triangulation (the 4 x 4 null vector) and
 * KeyFrame::UnprojectStereo (src/KeyFrame.cc:937-958) of either keyframe, the two depth tests, the two reprojection tests
 * (chi2 5.991 monocular, 7.8 stereo) and the scale-consistency test, for any number of keyframe pairs in one device round trip.
 * A problem is ONE (current keyframe, neighbour) pair with its match list.  Within one keyframe the neighbours are sequential --
 * a point created for neighbour k sets GetMapPoint(idx1), which SearchForTriangulation of neighbour k + 1 skips -- so a call
 * holds one problem per stream per round; the batch is across streams and whatever else the caller knows to be independent.
 * k_new_points: one lane per match, one wave per 64-match chunk of one problem, so the two cameras of a chunk are wave-uniform;
 * the host gathers the per-match operands by index while it packs; the Jacobi workspace lives in registers.
 * CONTRACT: status bytes and points of the device equal the library's host path (ORBX_NEWPOINTS=host in the environment, read
 * per call; host-only handles) and the numpy restatement tests/newpoints_model.py bit for bit, in both fp_modes.  Parity with an
 * OpenCV build is NOT pinned: DESIGN.md section 2 (F17) lists what follows the reference's source and what this library fixes
 * where the reference leaves it to OpenCV or libm (cv::SVD::compute, cv::norm, Mat::dot, the products, atan2f, cosf).
 * ComputeF12, the baseline / median-depth gate, AddObservation and Map::AddMapPoint stay the caller's.
 * Outputs are ragged in problem order, match order inside: status_out [sum nmatches], points_out [sum nmatches][3] (zeros for
 * every rejecting status; a stored NaN is the canonical quiet NaN).
 * DEVIATION: a feature with u_right >= 0 whose depth is not > 0 makes the reference dereference the empty cv::Mat that
 * UnprojectStereo returns; here a match with such a feature on either side gets ORBX_NEWPOINT_NO_DEPTH before any arithmetic.
 * Validated before any device work, ORBX_BAD_ARGUMENT: nproblems < 0, a null array whose size is positive, nmatches < 0, a
 * negative feature or level count, a match index outside its keyframe, an octave of a matched feature outside the scale tables.
 * nproblems == 0 and problems without a match succeed and launch nothing.
 * MEASURED on an MI355X (tools/newpoints_rate.py, profiles/newpoints_batch.md; n = 30 / 100 / 300 matches, against the
 * library's own host path on one core, which is neither the reference nor OpenCV): ONE problem per call takes 29 / 30 / 38 us
 * against 13 / 37 / 104 us, so a lone problem of 30 matches loses on the device; 16 per call 2.6 / 3.3 / 4.5 us each against
 * 10 / 34 / 101 us; 256 per call 0.39 / 3.1 / 8.8 us each.  compat/LocalMapping_newpoints.inl, one neighbour per call, runs the
 * host path below 100 matches. */
enum { ORBX_NEWPOINT_TRIANGULATED = 1,     /* accepted: x3D from the linear triangulation */
       ORBX_NEWPOINT_STEREO1 = 2,          /* accepted: mpCurrentKeyFrame->UnprojectStereo(idx1) */
       ORBX_NEWPOINT_STEREO2 = 3,          /* accepted: pKF2->UnprojectStereo(idx2) */
       ORBX_NEWPOINT_LOW_PARALLAX = 4,     /* the final else: no stereo and very low parallax */
       ORBX_NEWPOINT_ZERO_W = 5,           /* x3D.at<float>(3) == 0 */
       ORBX_NEWPOINT_DEPTH1 = 6,           /* z1 <= 0 */
       ORBX_NEWPOINT_DEPTH2 = 7,           /* z2 <= 0 */
       ORBX_NEWPOINT_REPROJ1 = 8,          /* the reprojection test in the current keyframe */
       ORBX_NEWPOINT_REPROJ2 = 9,          /* the reprojection test in the neighbour */
       ORBX_NEWPOINT_ZERO_DIST = 10,       /* dist1 == 0 || dist2 == 0 */
       ORBX_NEWPOINT_SCALE = 11,           /* the scale-consistency test */
       ORBX_NEWPOINT_NO_DEPTH = 12 };      /* u_right >= 0 without a positive depth (the library's own, see DEVIATION) */
typedef struct orbx_newpoints_keyframe {
    float Rcw[9], tcw[3], Ow[3];           /* GetRotation(), GetTranslation(), GetCameraCenter() as the keyframe holds them */
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
    int32_t nlevels;                       /* entries of the two tables */
    const float *scale_factors;            /* [nlevels] mvScaleFactors */
    const float *level_sigma2;             /* [nlevels] mvLevelSigma2 */
    int32_t n;                             /* features */
    const orbx_keypoint *keys_un;          /* [n] mvKeysUn */
    const float *keys;                     /* [n][2] mvKeys pt, the distorted positions UnprojectStereo reads */
    const float *u_right, *depth;          /* [n] mvuRight, mvDepth */
} orbx_newpoints_keyframe;
typedef struct orbx_newpoints_problem {
    orbx_newpoints_keyframe kf1, kf2;      /* mpCurrentKeyFrame, pKF2 */
    float scale_factor;                    /* mpCurrentKeyFrame->mfScaleFactor */
    int32_t nmatches;
    const int32_t *matches;                /* [nmatches][2] vMatchedIndices in order (idx1, idx2) */
} orbx_newpoints_problem;
/* One page-locked block up, k_new_points, one block down, the wait.  On a host-only handle the library's host path runs. */
orbx_status orbx_create_new_map_points_batch(orbx_handle *h, int nproblems, const orbx_newpoints_problem *problems,
                                             uint8_t *status_out, float *points_out);
/* cosParallaxStereo = cos(2 * atan2(mb / 2, depth)) as both paths get it for depth > 0 (csrc/orbx_newpoints.h).  Exported for
 * tests/newpoints_model.py, which takes this primitive from the library, and for the measurement of its distance from libm. */
float orbx_newpoints_stereo_cos(float mb, float depth);

/* ---- ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1433-1684) whole, pose algebra included, for any number of (KF1, KF2, Sim3)
 * problems in one device round trip: the SearchBySim3 stage of LoopClosing::ComputeSim3 (src/LoopClosing.cc:524-541) for every
 * candidate of a round.  A call touches nothing outside its own arguments (the reference rebuilds vpMapPointMatches before every
 * call), so the problems are independent.  The keyframes form a pool: each is uploaded and gridded ONCE, however many problems
 * name it (KF1 is mpCurrentKF for every candidate).
 * Arithmetic (csrc/orbx_sim3search.h, shared by host and device; the cv::Mat rule of tests/compat_runtime/opencv2/core/core.hpp):
 * sR12 = s12 R12 and sR21 = (1.0 / s12) R12^T element by element as (float)((double)elem * scalar); t21 = -sR21 t12, R p and
 * sR c with a double accumulator over k = 0, 1, 2 rounded once; the + t additions in float; `z < 0.0` rejects (z = +-0 goes on
 * to invz = +-inf and fails IsInImage); invz = (float)(1.0 / (double)z), x = X invz, y = Y invz; u = fx x + cx, v = fy y + cy
 * contracted to fmaf under ORBX_FP_GCC_FMA and rounded separately under ORBX_FP_STRICT; IsInImage is u >= minx && u < maxx &&
 * v >= miny && v < maxy; dist3D = (float)sqrt(double sum of squares in element order) against [0.8f min, 1.2f max]; the level of
 * orbx_predict_scale(max, dist3D); radius = th * scale[level]; level band [level - 1, level]; the winner is the first strict
 * minimum of the Hamming distance in GetFeaturesInArea visiting order and must be <= 100; the mutual test of :1667-1681.
 * Scale factors, level count and the PredictScale table come from the handle.
 * OUTPUTS: matches12[k][i1] (n of kf1 entries) = the KF2 feature whose MapPoint the reference writes into vpMatches12[i1], -1
 * where it leaves the entry alone; nfound[k] = the return value.
 * Debug rows (per problem, one entry per feature of kf1 / kf2; the struct and every field may be NULL): status (see the enum),
 * best = vnMatch1 / vnMatch2, level = nPredictedLevel where the point reached the search (else -1), uv = (u, v) where computed
 * (status >= 2; else zeros; a NaN is stored as the canonical quiet NaN).
 * CONTRACT: device = the library's host path (ORBX_SIM3SEARCH=host in the environment, read per call; host-only handles) =
 * tests/sim3_search_model.py, every output and debug field, in both fp_modes; matches and counts equal the reference's compiled
 * src/ORBmatcher.cc behind the stand-in cv::Mat (tests/test_sim3_search_cpu.py, tests/golden/sim3_search_*.json).  Parity with an
 * OpenCV build is not pinned.
 * Validated before any device work, ORBX_BAD_ARGUMENT: negative counts, a null field of a non-empty view, a null output row, kf1 /
 * kf2 outside the pool, an octave outside [0, nlevels), bad image bounds; ORBX_UNSUPPORTED: n > 65535.  nproblems == 0 launches
 * nothing; a call whose keyframes hold no feature at all has nothing to launch either and fills its (empty) outputs on the host. */
enum { ORBX_SIM3S_NOT_SEARCHED = 0,        /* no good point, or already matched */
       ORBX_SIM3S_BEHIND = 1,              /* z < 0 */
       ORBX_SIM3S_OUTSIDE = 2,             /* outside IsInImage */
       ORBX_SIM3S_DISTANCE = 3,            /* outside the distance band */
       ORBX_SIM3S_NO_CANDIDATE = 4,        /* empty window, or nothing in the level band */
       ORBX_SIM3S_TOO_FAR = 5,             /* best distance > 100 */
       ORBX_SIM3S_MATCH = 6 };             /* vnMatch set */
typedef struct orbx_sim3_search_keyframe {     /* host arrays; one entry per keyframe of the pool */
    int32_t n;
    const orbx_keypoint *keys_un;              /* mvKeysUn */
    const uint8_t *desc;                       /* mDescriptors, 32 per feature */
    float Tcw[16];                             /* row major; GetRotation() / GetTranslation() are read from it */
    const uint8_t *has_point;                  /* vpMapPoints[i] != NULL && !isBad() */
    const float *world_pos;                    /* GetWorldPos(), 3 per feature, read where has_point */
    const float *min_distance, *max_distance;  /* raw mfMinDistance / mfMaxDistance (0.8f / 1.2f applied inside) */
    const uint8_t *point_desc;                 /* MapPoint::GetDescriptor(), 32 per feature, read where has_point */
} orbx_sim3_search_keyframe;
typedef struct orbx_sim3_search_problem {
    int32_t kf1, kf2;                          /* indices into the pool; many problems may share kf1 */
    float s12, R12[9], t12[3], th;
    const uint8_t *matched1;                   /* n of kf1: vpMatches12[i] != NULL (NULL: none) */
    const uint8_t *matched2;                   /* n of kf2: vbAlreadyMatched2 as :1470-1483 compute it (NULL: none) */
} orbx_sim3_search_problem;
typedef struct orbx_sim3_search_debug {        /* one row pointer per problem; every field may be NULL */
    uint8_t *const *status1, *const *status2;
    int32_t *const *best1, *const *best2;
    int32_t *const *level1, *const *level2;
    float *const *uv1, *const *uv2;            /* 2 per feature */
} orbx_sim3_search_debug;
/* One page-locked block up, k_grid_build + k_sim3s_project + k_sim3s_cand + k_sim3s_mutual, one block down, the wait. */
orbx_status orbx_search_by_sim3_batch(orbx_handle *h, int nkeyframes, const orbx_sim3_search_keyframe *keyframes,
                                      int nproblems, const orbx_sim3_search_problem *problems, const float *camera4,
                                      const float *bounds4, int32_t *const *matches12, int *nfound,
                                      const orbx_sim3_search_debug *dbg);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */
