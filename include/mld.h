/*
 * mld.h — C-ABI of the MI355X-native DepthEstimator hot path.
 *
 * This is the drop-in boundary for monolidar_fusion's `Mono_Lidar::DepthEstimator`
 * (reference: monolidar_fusion/include/monolidar_fusion/DepthEstimator.h:39-359).
 * The reference has no FFI; its boundary is a C++ class.  Every entry point below names
 * the reference member it replaces.  The C++ shim class that keeps the reference's
 * method names on top of this ABI lives in
 * mono_lidar_depth_amd/host/monolidar_fusion/DepthEstimator.h; INTEGRATION.md shows how
 * a maintainer links it into tracklets_depth.
 *
 * Conventions
 *   - plain pointers and sizes only; caller-owned buffers; no callee resize.
 *   - return value: MLD_OK (0) or a negative mld_status; mld_last_error() gives the text
 *     (the reference throws `const char*` / std::string / std::runtime_error instead:
 *     DepthEstimator.cpp:38,57,94,227,270,439,608,797).
 *   - per-feature failures are never errors: (resultType, depth = -1), as in the reference
 *     (eDepthResultType.h:8-30).
 *   - one context per (GPU, stream).  A context owns `max_frames` independent frame slots so
 *     that many frames can be processed by ONE kernel launch set (frames of a sequence, or a
 *     micro-batch of sequences).  slot 0 alone gives the reference's one-frame-at-a-time use.
 *   - `*_device` entry points take device pointers (zero-copy: the cloud is read in place),
 *     are asynchronous on the context's stream, and never touch the host buffers.
 *   - threading: like a reference instance (mutable `_points`, DepthEstimator.h:300-334), a context serves one call
 *     at a time; different contexts are independent and may be driven from different host threads or processes
 *     (one per GPU).  mld_last_error / mld_create_error return thread-unsafe static text.
 *   - ordering with the caller's own GPU work: record/wait events on mld_get_stream() (see bench.py streaming_leg).
 */
#ifndef MLD_H_
#define MLD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLD_ABI_VERSION 8

typedef enum mld_status {
    MLD_OK = 0,
    MLD_ERR_INVALID_ARG = -1,        /* null pointer, bad slot, bad stride ...                         */
    MLD_ERR_NOT_INITIALIZED = -2,    /* "call of 'CalculateDepth' without 'SetInputCloud'" (:439)      */
    MLD_ERR_UNSUPPORTED_MODE = -3,   /* neighbor_search_mode != 0 (:57), region growing (:608), ...    */
    MLD_ERR_NO_ROAD_ESTIMATOR = -4,  /* "No road depth estimator selected." (:94)                      */
    MLD_ERR_NO_GROUND_PLANE = -5,    /* do_use_ransac_plane set but no plane supplied for the slot     */
    MLD_ERR_CLOUD_TOO_SMALL = -6,    /* GroundPlane::ExceptionPclInvalid (RansacPlane.cpp:44-50)       */
    MLD_ERR_HIP = -7,                /* a HIP runtime call failed; text in mld_last_error              */
    MLD_ERR_CAPACITY = -8            /* n / F / window larger than the context was created for (clouds: 8 388 607 points) */
} mld_status;

/* DepthResultType — monolidar_fusion/include/monolidar_fusion/eDepthResultType.h:8-30 (same values). */
typedef enum mld_result_type {
    MLD_Unspecified = 0,
    MLD_Success = 1,
    MLD_RadiusSearchInsufficientPoints = 2,
    MLD_HistogramNoLocalMax = 3,
    MLD_TresholdDepthGlobalGreaterMax = 4,
    MLD_TresholdDepthGlobalSmallerMin = 5,
    MLD_TresholdDepthLocalGreaterMax = 6,
    MLD_TresholdDepthLocalSmallerMin = 7,
    MLD_TriangleNotPlanar = 8,
    MLD_TriangleNotPlanarInsufficientPoints = 9,
    MLD_CornerBehindCamera = 10,
    MLD_PlaneViewrayNotOrthogonal = 11,
    MLD_PcaIsPoint = 12,
    MLD_PcaIsLine = 13,
    MLD_PcaIsCubic = 14,
    MLD_InsufficientRoadPoints = 15,
    MLD_SuccessRoad = 16,
    MLD_RegionGrowingNearestSeedNotAvailable = 17,
    MLD_RegionGrowingSeedsOutOfRange = 18,
    MLD_RegionGrowingInsufficientPoints = 19,
    MLD_SuccessRegionGrowing = 20,
    MLD_RESULT_TYPE_COUNT = 21
} mld_result_type;

/* CameraPinhole(width, height, f, cu, cv) — camera_pinhole.h:29-34. */
typedef struct mld_camera {
    double focal_length;
    double principal_point_x;
    double principal_point_y;
    int32_t width;
    int32_t height;
} mld_camera;

/*
 * The fields of DepthEstimatorParameters (DepthEstimatorParameters.h:7-173) that steer the hot
 * path and the per-frame ground-plane estimator, same names (including the reference's spelling).
 * Fields the path never reads (kd-tree, region growing, debug knobs) are not mirrored.
 * Layout: all doubles first, then int32s — no implicit padding except the tail.
 */
typedef struct mld_params {
    double histogram_segmentation_bin_witdh;     /* :43  */
    double treshold_depth_local_value;           /* :92  */
    double pca_treshold_3_abs_min;               /* :102 */
    double pca_treshold_3_2_rel_max;             /* :103 */
    double pca_treshold_2_1_rel_min;             /* :104 */
    double ransac_plane_point_distance_treshold; /* :122 */
    double ransac_plane_distance_treshold;       /* :114  RANSAC inlier distance (ground-plane estimation) */
    double ransac_plane_min_z;                   /* :115 */
    double ransac_plane_max_z;                   /* :116 */
    double ransac_plane_refinement_treshold;     /* :119 */
    double ransac_plane_probability;             /* :124 */
    double plane_estimator_z_x_min_relation;     /* :141 */
    double triangleplanar_crossnorm_treshold;    /* :154 */
    double viewray_plane_orthoganality_treshold; /* :155 */
    double ransac_plane_treshold_camx;           /* :121  |x_cam| bound of the ground-plane debug cloud */
    int32_t neighbor_search_mode;                /* :20  must be 0 */
    int32_t pixelarea_search_witdh;              /* :21  */
    int32_t pixelarea_search_height;             /* :22  */
    int32_t radiusSearch_count_min;              /* :35  */
    int32_t do_use_histogram_segmentation;       /* :42  */
    int32_t histogram_segmentation_min_pointcount; /* :44 */
    int32_t do_use_depth_segmentation;           /* :48  must be 0 (reference throws, DepthEstimator.cpp:608); the mode
                                                  *      itself, for a batch: mld_row_growth below */
    int32_t treshold_depth_enabled;              /* :78  */
    int32_t treshold_depth_mode;                 /* :79  0 Dispose, 1 Adjust */
    int32_t treshold_depth_max;                  /* :80  (int in the reference) */
    int32_t treshold_depth_min;                  /* :81  */
    int32_t treshold_depth_local_enabled;        /* :89  */
    int32_t treshold_depth_local_mode;           /* :90  */
    int32_t treshold_depth_local_valuetype;      /* :91  0 absolute, 1 relative */
    int32_t do_use_PCA;                          /* :100 */
    int32_t do_use_ransac_plane;                 /* :113 */
    int32_t plane_estimator_use_triangle_maximation; /* :140 */
    int32_t plane_estimator_use_leastsquares;    /* :142 (Ceres variant: unsupported, UB in the reference) */
    int32_t plane_estimator_use_mestimator;      /* :143 */
    int32_t do_use_cut_behind_camera;            /* :151 */
    int32_t do_use_triangle_size_maximation;     /* :152 */
    int32_t do_check_triangleplanar_condition;   /* :153 */
    int32_t set_all_depths_to_zero;              /* :156 */
    int32_t ransac_plane_max_iterations;         /* :117 */
    int32_t ransac_plane_use_refinement;         /* :118 */
    int32_t ransac_plane_use_camx_treshold;      /* :120 */
} mld_params;

/* Header defaults of DepthEstimatorParameters.h (note viewray_plane_orthoganality_treshold{01} == 1.0). */
void mld_params_default(mld_params* p);
/* "C0": monolidar_fusion/parameters.yaml with do_use_depth_segmentation: 0. */
void mld_params_c0(mld_params* p);
/* DepthEstimatorParameters::fromFile (DepthEstimatorParameters.cpp:16-114): `key: value` YAML subset, cv::FileStorage
 * semantics: an absent key reads as 0, `(int)node` rounds to nearest (saturating here).  On failure `err` holds the
 * reason; on success it holds a note listing the mirrored keys the file lacks ("absent (read as 0): a, b", or ""). */
int mld_params_from_file(mld_params* p, const char* path, char* err, int err_len);

typedef struct mld_ctx mld_ctx;

int mld_abi_version(void);

/*
 * InitConfig + Initialize (DepthEstimator.cpp:35-154).
 *   T_cam_lidar: row-major 3x4 [R|t] of the lidar->camera Affine3d.
 *   max_frames:  number of frame slots (>=1).  max_points / max_features: per-slot capacities for
 *   the host-pointer entry points (device-pointer entry points borrow the caller's buffers).
 * Returns NULL on failure; *status_out (optional) receives the reason, and
 * mld_create_error() the text.
 */
mld_ctx* mld_create(const mld_params* params, const mld_camera* camera, const double T_cam_lidar[12],
                    int device, int max_frames, int64_t max_points, int64_t max_features, int* status_out);
const char* mld_create_error(void);
void mld_destroy(mld_ctx* ctx);
const char* mld_last_error(const mld_ctx* ctx);

/* The hipStream_t the context launches on (as void*), for callers that order their own work. */
void* mld_get_stream(mld_ctx* ctx);

/*
 * Do the streams of two contexts execute side by side?  1 = yes; 0 = they share a hardware queue of the HIP runtime
 * (their kernels run strictly in turn: mld_order_after[_classify] / mld_set_shared_gpu then buy nothing) or are the same
 * context; < 0 = error.  The runtime multiplexes a process's streams on a few hardware queues (four per priority unless
 * GPU_MAX_HW_QUEUES says otherwise), so mld_create probes a new context's stream against every live context of its device
 * and replaces it until it has a queue of its own (up to six tries); this call repeats the probe on demand (both streams
 * are synchronised, two one-wavefront kernels run: ~50 us; 3 ms when the answer is 0).  No reference counterpart.
 */
int mld_contexts_concurrent(mld_ctx* a, mld_ctx* b);
int mld_synchronize(mld_ctx* ctx);

/*
 * Two (or more) contexts on one GPU, used alternately ("double buffering"; DESIGN.md §4 "Batches").
 * The projection kernel streams the clouds from HBM; the feature kernels wait for scattered fetches and move a tenth of
 * the bytes.  Run beside each other they finish sooner than one after the other (HBM busy 0.8 of the step instead of
 * 0.6) -- the reference has no counterpart: its stage A is serial and its feature loop is the only
 * parallel part (DepthEstimator.cpp:156-217 vs :455).  Schedule per batch, contexts taken round-robin:
 *     mld_set_clouds_*_device(ctx_k, ...);      projection of batch i on context k
 *     mld_order_after(ctx_next, ctx_k);          the NEXT context's projection starts when this one is done ...
 *       (or mld_order_after_classify: ... when this context's classification kernel is done)
 *     mld_calculate_depths_device(ctx_k, ...);   ... i.e. beside these feature kernels
 *
 * mld_order_after: everything submitted to `ctx` from now on starts after everything submitted to `other` so far has
 *   finished (one event; no host synchronisation).  Both contexts must live on the same device.
 * mld_set_shared_gpu(ctx, 1): the lane-per-feature kernel of `ctx` keeps to ten wavefronts per CU instead of sixteen (it
 *   requests more LDS per block), which leaves registers for the other context's projection wavefronts on every CU.  A
 *   context that has the GPU to itself is ~20 % slower in this mode; the alternating pair is ~20 % faster (bench.py
 *   default: 0.68-0.72 instead of 0.89 ms per 1024 frames of config 2).  `shared`: bit 0 = on; bits 8..15 = wavefronts of
 *   the lane-per-feature kernel per CU in that mode (0 = the default, 10): fewer leave more of every CU to the projection.
 */
int mld_order_after(mld_ctx* ctx, mld_ctx* other);
/*
 * mld_order_after_classify: the same hand-over, but it is `ctx`'s next PROJECTION KERNEL (and what follows it) that waits -
 *   the bitmap fill and descriptor upload queued ahead of that kernel do not -, and it is released behind the
 *   classification kernel of `other`'s NEXT mld_calculate_depth(s)_device call instead of at once: the classification
 *   (one 1024-thread block and 63 KB of LDS per frame, 40 us per 1024 frames) then has the GPU to itself instead of competing with 131 072 projection blocks for wave
 *   slots, and the projection of `ctx` still runs beside the long feature kernels (measured: k_classify 70-90 -> 44 us,
 *   the step 0.5-1.5 % shorter and steadier; LAB.md 4.17).  The release itself is a one-wavefront kernel (k_gate) queued
 *   in front of the projection that polls a counter of the classification blocks that have been placed on a CU - once the
 *   last one runs, nothing of that kernel still waits for wave slots or LDS (LAB.md 5.29) - 2-3 us from there to the
 *   projection's start instead of the ~15 us of a cross-stream event (LAB.md 4.28); its polling is bounded (it gives up
 *   after 100 000 polls, a fraction of a second), because nothing depends on it: purely a scheduling hint, the contexts share no data.  Nothing waits if
 *   `other` never issues that call; a pending hand-over ends with either context.
 */
int mld_order_after_classify(mld_ctx* ctx, mld_ctx* other);
/*
 * mld_pair_contexts(a, b): the batched setInputCloud entry points (mld_set_clouds_*_device) of BOTH contexts run their
 *   projection on one stream created here (owned by `a`), back to back in call order, while each context's feature
 *   kernels stay on its own stream (two events per batch join them).  With the schedule above this replaces
 *   mld_order_after: the projection of batch i+1 follows that of batch i without a cross-stream hand-over (~50 us per
 *   1024-frame batch) and still runs beside the feature kernels of batch i.  A projection waits for everything queued on
 *   its own context before (the kernels still reading the slots' maps).  Destroy `b` before `a`.
 */
int mld_pair_contexts(mld_ctx* a, mld_ctx* b);
int mld_set_shared_gpu(mld_ctx* ctx, int shared);
/*
 * Capacities (entries per feature) of the lane-per-feature kernel's two neighbour lists: the scanned window (the road
 * window, 2.0 x 1.5 the search window, when the fallback is on) and the narrow search window.  Features whose lists are
 * longer are handled by the wave-cooperative kernel (same results, ~10x the cost per feature).  Default 32 / 24: right
 * for 64-beam clouds (config 2: 11 / 2.3 neighbours on average).  Dense clouds (128 beams x 4096: 16 / 6 on average, 48
 * at most in the road window) want 48 / 24: BASELINE config 5 at batch size runs 1.8x faster with it.  LDS per wavefront
 * = (wide + narrow) * 256 bytes unless mld_set_list_budget lowers it.  8 <= narrow <= wide <= 64.  Capacities beyond the default also select the kernel's
 * DENSE instantiations: the corner search over the segmented points and the histogram's depths in registers - up to 24 of
 * each at two wavefronts per SIMD when the context has the GPU to itself, up to 16 inside 168 registers when
 * mld_set_shared_gpu is on, so that another context's projection finds room beside it (config 5 at 256 sequences per
 * step: 1.12 G associations/s in round 4 -> 1.85 G with one context, 1.98 G with two in turn).
 */
int mld_set_list_capacity(mld_ctx* ctx, int wide_entries, int narrow_entries);

/*
 * LDS entries per feature that the two lists SHARE (the narrow lists of a wavefront's 64 features are stored behind the
 * longest of their wide lists): a feature stays on the lane-per-feature kernel when wide <= wide capacity, narrow <= narrow
 * capacity and (longest wide list of its wavefront) + narrow <= total.
 * LDS per wavefront = total * 256 bytes, which sets how many wavefronts of the kernel a CU holds (160 KB / that, at most
 * four per SIMD).  A new context: capacities 32 / 24, budget 40 (10 KB, 16 wavefronts per CU; on 64-beam and 16-beam
 * clouds no list pair comes near it: wide + narrow <= 27 on BASELINE configs 2 and 3).  mld_set_list_capacity resets the
 * budget to wide + narrow (both lists at their longest: the dense 128-beam clouds of config 5 reach 66 of 48 + 24).
 * wide capacity <= total_entries <= wide + narrow capacity; 0 = wide + narrow.
 */
int mld_set_list_budget(mld_ctx* ctx, int total_entries);

/*
 * setInputCloud (DepthEstimator.cpp:220-312): projection + pixel->point map for one slot.
 *   pts: x,y,z[,..] float32 records, stride_bytes 16 (packed xyzi) or 32 (pcl::PointXYZI layout,
 *   DepthEstimator.cpp:169 reads rows 0-2 of the 8-float map).
 */
int mld_set_cloud(mld_ctx* ctx, int slot, const void* pts_host, int64_t n, int stride_bytes);
int mld_set_cloud_device(mld_ctx* ctx, int slot, const void* pts_dev, int64_t n, int stride_bytes);
/* All slots [0, n_slots) in ONE launch; pts_dev[i] / n[i] are host arrays of device pointers / counts. */
int mld_set_clouds_device(mld_ctx* ctx, int n_slots, const void* const* pts_dev, const int64_t* n,
                          int stride_bytes);
/*
 * Host-side staging for callers that stream frames through (pinned) upload buffers: copies n records of
 * src_stride_bytes (32: pcl::PointXYZI as the reference's caller holds them, DepthEstimator.h:62-63; or 16) into packed
 * 16-byte records {x, y, z, intensity} at dst16, with up to n_threads host threads (one per ~64 K points).  The copy a
 * driver makes anyway then halves what crosses PCIe, the bound of the streamed path.  No GPU call; no context.
 */
int mld_pack_points_host(void* dst16, const void* src, int64_t n, int src_stride_bytes, int n_threads);

/*
 * setInputCloud(cloud, groundPlane) with an already segmented plane (DepthEstimator.cpp:220-312, :281: nothing to
 * estimate) for slots [0, n_slots) in ONE launch: coeffs is n_slots x 4 (host), mask_dev a host array of device
 * bitmask pointers (bit i of word i/32 = point i is an inlier, the device form of `_pointIsInPlane`,
 * RansacPlane.h:116-122).  Because the plane is known when the cloud is projected, every pixel-map entry carries
 * its point's inlier flag and the road fallback needs no mask lookups.  Equivalent to mld_set_clouds_device +
 * mld_set_ground_planes_mask_device, which remain for planes that arrive after the cloud.
 */
int mld_set_clouds_planes_device(mld_ctx* ctx, int n_slots, const void* const* pts_dev, const int64_t* n,
                                 int stride_bytes, const float* coeffs, const uint32_t* const* mask_dev);

/*
 * setInputCloud(cloud, groundPlane) with a plane that is NOT segmented yet — the reference's default call — for slots
 * [0, n_slots) in one asynchronous launch set: RansacPlane::CalculateInliersPlane (RansacPlane.cpp:41-140) runs for
 * every slot on the GPU (one block per slot), the planes stay in device memory where the projection (inlier flags in
 * the map keys) and the feature kernels read them; nothing returns to the host.  seeds: one per slot (the reference's
 * pcl::RandomSample is time-seeded).  A slot whose estimation fails (GroundPlane::ExceptionPclInvalid, which the
 * caller of the reference catches, tracklet_depth_module.cpp:321,338) runs without the road fallback.
 * mld_get_estimated_planes returns coefficients / inlier counts / status (0 ok, 1 failed) and synchronises; the inlier
 * sets are available through mld_get_ground_plane_inliers.
 */
int mld_set_clouds_estimate_planes_device(mld_ctx* ctx, int n_slots, const void* const* pts_dev, const int64_t* n,
                                          int stride_bytes, const uint32_t* seeds);
int mld_get_estimated_planes(mld_ctx* ctx, int n_slots, float* coeffs_out, int64_t* n_inliers_out, int32_t* status_out);

/*
 * The GroundPlane object handed to setInputCloud/CalculateDepth (RansacPlane.h:38-123):
 * coefficients a,b,c,d in the LIDAR frame + the inlier index set keyed by ORIGINAL cloud index
 * (`_pointIsInPlane`, RansacPlane.h:116-122).  coeffs == NULL: "ransacPlane == nullptr"
 * (road fallback skipped, DepthEstimator.cpp:580).  Must be called after the slot's cloud is set.
 */
int mld_set_ground_plane(mld_ctx* ctx, int slot, const float coeffs[4], const int32_t* inlier_idx_host,
                         int64_t n_inliers);
int mld_set_ground_plane_device(mld_ctx* ctx, int slot, const float coeffs[4], const int32_t* inlier_idx_dev,
                                int64_t n_inliers);
/*
 * RansacPlane::CalculateInliersPlane on the GPU (monolidar_fusion/src/RansacPlane.cpp:41-140) — what setInputCloud
 * runs when the GroundPlane handed in is not segmented yet (DepthEstimator.cpp:275-283).  Estimates the plane of
 * the slot's cloud (parameters ransac_plane_*), installs it as the slot's ground plane and returns the
 * coefficients and the inlier count.  `seed` makes the random draws reproducible (the reference is time-seeded).
 * Synchronises.  MLD_ERR_CLOUD_TOO_SMALL: fewer than 3 usable points / no model (ExceptionPclInvalid).
 */
int mld_estimate_ground_plane(mld_ctx* ctx, int slot, uint32_t seed, float coeffs_out[4], int64_t* n_inliers_out);
/*
 * SemanticPlane::CalculateInliersPlane on the GPU (monolidar_fusion/src/RansacPlane.cpp:195-274) — the ground plane
 * tracklets_depth uses when a semantic label image accompanies the frame (tracklet_depth_module.cpp:270-284):
 * points whose projection falls on a pixel with a ground label (:198-221), least-squares plane through them
 * (:238-246), all cloud points within `inlier_threshold` of it (:252), plane refitted to those (:253); installs the
 * result as the slot's ground plane (coefficients of the refit, inliers = the selected points, :259-268).
 * SemanticPlane::Camera is the context's own calibration (f, cu, cv, T_cam_lidar), as the caller builds it.
 * label_image: rows x cols uint8, row_stride_bytes apart.  Fewer than 3 labelled points: MLD_ERR_CLOUD_TOO_SMALL
 * (ExceptionPclInvalid, :224-227).  Pixels x == cols / y == rows, which the reference reads out of bounds, carry no
 * label here.  PCL's sequential float sums are replaced by 256 interleaved partial sums (parity unpinned, as for
 * mld_estimate_ground_plane).
 */
int mld_estimate_semantic_plane(mld_ctx* ctx, int slot, const uint8_t* label_image_host, int rows, int cols,
                                int row_stride_bytes, const int32_t* ground_labels, int n_labels, double inlier_threshold,
                                float coeffs_out[4], int64_t* n_inliers_out);
int mld_estimate_semantic_plane_device(mld_ctx* ctx, int slot, const uint8_t* label_image_dev, int rows, int cols,
                                       int row_stride_bytes, const int32_t* ground_labels, int n_labels,
                                       double inlier_threshold, float coeffs_out[4], int64_t* n_inliers_out);
/* The slot's current inlier set as ascending original indices (GroundPlane::getInlinersIndex). */
int mld_get_ground_plane_inliers(mld_ctx* ctx, int slot, int32_t* index_out, int64_t capacity, int64_t* n_out);
/* Same, with the inlier set already as a device bitmask (bit i of word i/32 = point i is an inlier). */
int mld_set_ground_plane_mask_device(mld_ctx* ctx, int slot, const float coeffs[4], const uint32_t* mask_dev);
/* Slots [0, n_slots): coeffs is n_slots x 4 (host), mask_dev a host array of device bitmask pointers. */
int mld_set_ground_planes_mask_device(mld_ctx* ctx, int n_slots, const float* coeffs, const uint32_t* const* mask_dev);

/*
 * CalculateDepth(Matrix2Xd, VectorXd&, VectorXi&, GroundPlane::Ptr) (DepthEstimator.cpp:429-488).
 *   uv: 2 x F column-major (u0,v0,u1,v1,...) float64, as Eigen::Matrix2Xd stores it.
 *   depth_out: F float64 (metres, camera-frame z of the intersection, -1 on failure);
 *   type_out: F int32 mld_result_type (may be NULL: the overload without resultType, :422-427).
 * The host-pointer form copies in, runs, copies out and synchronises.
 */
int mld_calculate_depth(mld_ctx* ctx, int slot, const double* uv_host, int64_t F, double* depth_out_host,
                        int32_t* type_out_host);
/* flags of mld_calculate_depth_opts */
#define MLD_CALC_SKIP_ROAD 1u /* this call only: "ransacPlane == nullptr" (DepthEstimator.cpp:580), the slot's plane stays */
int mld_calculate_depth_opts(mld_ctx* ctx, int slot, const double* uv_host, int64_t F, double* depth_out_host,
                             int32_t* type_out_host, uint32_t flags);
int mld_calculate_depth_device(mld_ctx* ctx, int slot, const double* uv_dev, int64_t F, double* depth_out_dev,
                               int32_t* type_out_dev);
/*
 * CalculateDepth(cloud, uv, depths, resultType, groundPlane) (DepthEstimator.cpp:404-420: setInputCloud followed by
 * the per-feature loop) for ONE frame held in host memory, in a single call: mld_set_cloud + mld_set_ground_plane +
 * mld_calculate_depth with the small transfers combined and the plane installed before the projection.  The one-frame
 * latency path of a ROS callback (tracklet_depth_module.cpp:63-117).  coeffs == NULL: no plane (road fallback off).
 * Synchronises.  type_out may be NULL.
 */
int mld_calculate_depth_frame(mld_ctx* ctx, int slot, const void* pts_host, int64_t n, int stride_bytes,
                              const float coeffs[4], const int32_t* inlier_idx_host, int64_t n_inliers,
                              const double* uv_host, int64_t F, double* depth_out_host, int32_t* type_out_host);
/*
 * The same single call for the reference's PRODUCTION use: the GroundPlane handed to CalculateDepth(cloud, uv, depths,
 * types, groundPlane) is NOT segmented yet - TrackletDepthModule::process builds a fresh one for every frame
 * (tracklet_depth_module.cpp:269-284) and setInputCloud estimates it (DepthEstimator.cpp:275-283) before the feature loop
 * runs.  One asynchronous chain on the context's stream, no host round trip before the result:
 *     H2D (cloud, features, label image) -> plane estimation on the slot (RansacPlane::CalculateInliersPlane,
 *     RansacPlane.cpp:41-140, one block; or SemanticPlane::CalculateInliersPlane, :195-274) -> projection WITH that plane
 *     (the points' ground-plane state rides in the pixel-map keys) -> feature kernel -> one D2H (depths, types, plane)
 * The estimated plane stays installed on the slot (later mld_calculate_depth calls use it); its inlier index list is
 * not produced here - mld_get_ground_plane_inliers fetches it on demand (GroundPlane::getInlinersIndex).
 *   plane->kind MLD_PLANE_RANSAC:   `seed` fixes the draws (the reference's pcl::RandomSample is time-seeded)
 *   plane->kind MLD_PLANE_SEMANTIC: label_image (HOST memory, rows x cols uint8, row_stride_bytes apart), ground_labels,
 *                                   inlier_threshold as mld_estimate_semantic_plane
 *   plane_out (optional): coefficients, inlier count, status 0 / 1, RANSAC iterations.
 * Without do_use_ransac_plane the plane request is ignored (as setInputCloud does, :274).  A failed estimation
 * (GroundPlane::ExceptionPclInvalid: fewer than 3 usable points / no model) returns MLD_ERR_CLOUD_TOO_SMALL and leaves
 * depth_out / type_out untouched - the reference throws out of setInputCloud before any depth is computed
 * (tracklet_depth_module.cpp:321,338 catch it).  Synchronises.  type_out may be NULL.
 */
#define MLD_PLANE_RANSAC 0
#define MLD_PLANE_SEMANTIC 1
typedef struct mld_plane_request {
    int32_t kind;
    uint32_t seed;
    const uint8_t* label_image;
    int32_t rows, cols, row_stride_bytes;
    int32_t n_labels;
    const int32_t* ground_labels;
    double inlier_threshold;
} mld_plane_request;
typedef struct mld_plane_result {
    float coeffs[4];
    int64_t n_inliers;
    int32_t status;      /* 0 ok, 1 = ExceptionPclInvalid */
    int32_t iterations;  /* RANSAC iterations PCL's stopping rule counted (0 for the semantic plane) */
} mld_plane_result;
int mld_calculate_depth_frame_estimate(mld_ctx* ctx, int slot, const void* pts_host, int64_t n, int stride_bytes,
                                       const mld_plane_request* plane, const double* uv_host, int64_t F,
                                       double* depth_out_host, int32_t* type_out_host, mld_plane_result* plane_out);
/*
 * Where the time of the LAST one-frame call (mld_calculate_depth_frame / _frame_estimate) went.  The host-clock entries
 * ([4]-[6], [8], [9]) are always filled; the GPU phases ([0]-[3], [7]) only when timing is enabled (mld_timing_enable: the
 * hipEvents that bracket the phases cost the call tens of microseconds, so the un-instrumented call is faster than their
 * sum) and are 0 otherwise.  out_us[10]:
 *   [0] h2d      cloud copy on the context's stream (the small inputs travel beside it on a side stream)
 *   [1] plane    plane estimation kernels (0 for a supplied plane)
 *   [2] kernels  projection + feature kernel(s)
 *   [3] d2h      result copy
 *   [4] api      host time to enqueue everything (entry -> last enqueue returned)
 *   [5] wait     host time blocked in the final synchronise
 *   [6] total    host wall time of the call
 *   [7] gpu      first event -> last event on the stream ([0]+[1]+[2]+[3] plus the gaps between them)
 *   [8] pre      host time before the cloud copy is submitted (validation, staging of the small inputs, side-stream work)
 *   [9] copycall host time inside the cloud's hipMemcpyAsync (a pageable source blocks until it is staged)
 */
int mld_frame_timing(mld_ctx* ctx, double out_us[10]);
/* All slots [0, n_slots) in ONE launch set (host arrays of device pointers / counts). */
int mld_calculate_depths_device(mld_ctx* ctx, int n_slots, const double* const* uv_dev, const int64_t* F,
                                double* const* depth_out_dev, int32_t* const* type_out_dev);

/*
 * Tracklet gather / scatter either side of the path — TrackletDepthModule::process
 * (tracklets_depth/src/tracklet_depth_module.cpp:23-61 ExractNewTrackletFrames, :63-117 CalculateFeatureDepths*,
 * :119-169 SaveFeatureDepths).  For n_tracks tracks:
 *   u_new/v_new : newest feature of every track            (feature_points.at(0), float32 as in the message)
 *   u_old/v_old : previous feature (feature_points.at(1)); read only where is_new[i] != 0
 *   is_new      : the track id is not yet in the tracklet map (a new tracklet contributes TWO features)
 * Features are truncated to integer pixels as the reference's std::pair<int,int> does.  The current frame's
 * features are evaluated on `slot_cur`, the previous features of NEW tracks on `slot_last` — the previous frame's
 * slot, whose projection and pixel map are still resident (no re-projection); slot_last = -1: no previous cloud,
 * those depths are -1 (:93-96).  Both slots must have their cloud (and ground plane) set.
 *   d_cur_out  : n_tracks float32 depths of the newest features            (FeaturePoint.d)
 *   d_last_out : n_tracks float32; written only where is_new[i] != 0
 *   type_*_out : optional int32 result types, same indexing
 *   n_new_host : optional; receives the number of new tracks (synchronises)
 * The `_device` form takes device pointers and is asynchronous on the context's stream.
 */
int mld_tracklets_depth_device(mld_ctx* ctx, int slot_cur, int slot_last, const float* u_new, const float* v_new,
                               const float* u_old, const float* v_old, const uint8_t* is_new, int64_t n_tracks,
                               float* d_cur_out, float* d_last_out, int32_t* type_cur_out, int32_t* type_last_out,
                               int64_t* n_new_host);
int mld_tracklets_depth(mld_ctx* ctx, int slot_cur, int slot_last, const float* u_new, const float* v_new,
                        const float* u_old, const float* v_old, const uint8_t* is_new, int64_t n_tracks,
                        float* d_cur_out, float* d_last_out, int32_t* type_cur_out, int32_t* type_last_out,
                        int64_t* n_new_host);
/*
 * TrackletDepthModule::process (tracklet_depth_module.cpp:261-396) for ONE frame held in host memory as a single call -
 * the ROS callback's whole GPU side: setInputCloud of the new cloud on `slot_cur` with its ground plane (`plane`: not
 * segmented yet, estimated on the GPU inside the call as in mld_calculate_depth_frame_estimate - what the reference's
 * process() does every frame; or plane == NULL and coeffs / inliers: a segmented plane; both NULL: no plane), the
 * feature marshalling, both CalculateDepth calls (the previous frame from its resident `slot_last`, -1: none) and the
 * float32 scatter of mld_tracklets_depth.  One asynchronous chain, one synchronisation; track arrays and results travel in
 * one pinned block each way.  Arrays and outputs as mld_tracklets_depth.  A failed plane estimation
 * (GroundPlane::ExceptionPclInvalid) returns MLD_ERR_CLOUD_TOO_SMALL with d_cur_out = -1 and d_last_out answered from
 * the previous frame, as the reference's two try blocks do (:318-347).
 */
int mld_tracklets_frame(mld_ctx* ctx, int slot_cur, int slot_last, const void* pts_host, int64_t n, int stride_bytes,
                        const mld_plane_request* plane, const float coeffs[4], const int32_t* inlier_idx_host,
                        int64_t n_inliers, const float* u_new, const float* v_new, const float* u_old, const float* v_old,
                        const uint8_t* is_new, int64_t n_tracks, float* d_cur_out, float* d_last_out, int32_t* type_cur_out,
                        int32_t* type_last_out, int64_t* n_new_host, mld_plane_result* plane_out);
/*
 * The tracklet layer at batch size: the current frames of n_seq independent SEQUENCES in one launch set
 * (TrackletDepthModule::process, tracklet_depth_module.cpp:261-396, once per sequence).  The context's frame slots are
 * used as two banks of n_seq slots (create the context with max_frames >= 2 * n_seq): sequence s keeps its current
 * frame in slot bank_cur * n_seq + s and its previous frame, still resident, in slot (1 - bank_cur) * n_seq + s; the
 * caller flips bank_cur every frame.
 *   mld_set_clouds_planes_range_device  setInputCloud(cloud, plane) for the slots [first_slot, first_slot + n_slots)
 *                                       (coeffs / mask_dev: both or neither), i.e. for one bank
 *   mld_tracklets_depths_device         gather -> depth of every track's newest feature on the current frame and of the
 *                                       NEW tracks' previous features on the previous frame (have_last == 0: no previous
 *                                       clouds yet, those depths are -1) -> float32 scatter; arrays of n_seq device
 *                                       pointers / counts, indexing and meaning per sequence as mld_tracklets_depth_device
 *   mld_tracklets_depths_lanes_device   the same with have_last[s] (host, n_seq flags) per sequence, for sequences that
 *                                       start at different frames: where have_last[s] == 0 nothing of the previous-bank
 *                                       slot of s is read and the new tracks of s get d_last = -1 / MLD_Unspecified - what
 *                                       the scalar flag does for all sequences.  Equal flags: the scalar call.  Mixed
 *                                       flags: two launch sets of the scalar call, the sequences with a previous frame,
 *                                       then those without, each with the other group's track counts at zero.
 *                                       DEVIATION: with mixed flags the previous-bank slot of EVERY sequence is checked
 *                                       as the scalar call checks it (a cloud, and a plane where the parameters ask for
 *                                       one), also where have_last[s] == 0 and nothing of it is read: such a slot must
 *                                       have held some frame (TrackletBatch gives a slot that never did the current
 *                                       one).  The flags are consumed before the call returns.
 * Asynchronous on the context's stream; per-sequence results equal n_seq single-sequence calls.
 */
int mld_set_clouds_planes_range_device(mld_ctx* ctx, int first_slot, int n_slots, const void* const* pts_dev,
                                       const int64_t* n, int stride_bytes, const float* coeffs,
                                       const uint32_t* const* mask_dev);
int mld_tracklets_depths_device(mld_ctx* ctx, int n_seq, int bank_cur, int have_last, const float* const* u_new,
                                const float* const* v_new, const float* const* u_old, const float* const* v_old,
                                const uint8_t* const* is_new, const int64_t* n_tracks, float* const* d_cur_out,
                                float* const* d_last_out, int32_t* const* type_cur_out, int32_t* const* type_last_out);
int mld_tracklets_depths_lanes_device(mld_ctx* ctx, int n_seq, int bank_cur, const uint8_t* have_last, const float* const* u_new,
                                      const float* const* v_new, const float* const* u_old, const float* const* v_old,
                                      const uint8_t* const* is_new, const int64_t* n_tracks, float* const* d_cur_out,
                                      float* const* d_last_out, int32_t* const* type_cur_out, int32_t* const* type_last_out);

/*
 * The tracklet map of the batched layer, resident on the GPU — `_trackletMap` (std::map<int, feature_tracking::Tracklet>,
 * a deque of (u, v, depth) per id) and the four places of TrackletDepthModule::process that touch it, for n_seq
 * independent sequences per call:
 *   mld_tracks_begin_device   ExractNewTrackletFrames' membership test `_trackletMap.count(id)`
 *                             (tracklet_depth_module.cpp:23-61, :31): which ids of this frame are new
 *   mld_tracks_commit_device  SaveFeatureDepths (:119-169) + TidyUpTracklets (:171-193) for the frame begun
 *   mld_tracks_export_device  convert_tracklets_to_matches_msg (:209-259): the stored tracks in message order
 *   mld_tracks_export_packed_device  the same tracks back to back, every track with exactly its stored entries, and
 *                             the offsets at which they start (what the message holds: `curTracklet.size()` points each)
 *   mld_tracks_export_leaving_device  between a begin and its commit: the tracks TidyUpTracklets is about to erase, whole,
 *                             and the entries the max_history cap is about to drop; mld_tracks_set_leaving_sink: the same
 *                             from inside the next step call
 *   mld_tracks_import_packed_device  the inverse of the packed export: the committed frame of the selected sequences
 *                             replaced by given tracks, as if a fresh TrackletDepthModule had been brought to that state
 *                             (the reference has no checkpoint / resume: SURVEY 5); mld_tracks_reset_device: by no tracks
 *   mld_tracks_counts         the counters those functions return ((new, old) :60/:168, (success, failed) :258)
 *   mld_tracklets_step_device begin -> mld_tracklets_depths_device with the store's masks -> commit: process()'s whole
 *                             track side (:286-347) as ONE asynchronous chain; ids + features in, depths + histories out
 *   mld_tracklets_step_lanes_device  the same for sequences that start, restart and resume independently: have_last
 *                             and restart per sequence
 * The store is bound to a context: it lives on that context's device and every call is asynchronous on that context's
 * stream (mld_tracks_counts synchronises).  The host tables (arrays of n_seq device pointers / counts) are consumed
 * before a call returns: a caller may queue many frames ahead of the device and reuse its host arrays.  The device
 * arrays must stay valid until the work has run; the ids of a frame are read by its begin AND its commit.
 * Like a context, a store serves one call at a time.
 *
 * mld_tracks_create: one map per sequence.
 *   max_tracks : tracks per frame and sequence the store sustains indefinitely at any churn (every track replaced
 *                every frame included): the rows of the tracks that ended are taken back before new ones are handed out.
 *   max_history: >= 2; stored entries per track.  DEVIATION: the reference's deque is unbounded, here the oldest entries
 *                fall off - results equal the reference whenever no track outlives max_history frames.  An archive that
 *                takes mld_tracks_export_leaving_device's spilled entries before every commit loses nothing.
 *   All memory is allocated here, none per frame.  Device bytes with cap = the power of two >= 2 * max_tracks:
 *     n_seq * (max_tracks * (12 * max_history + 45) + 16 * cap + 132 + 12 * ceil(max_tracks / 256))
 *   (histories 12 * max_history per track: 0.49 GB of 0.74 GB for 256 sequences x 10 000 tracks x 16 entries; 4 of the 45
 *   bytes per track and the last term are the scratch of the packed export's scan: length and ring head per track, a
 *   32-bit sum and a 64-bit base per block of 256 tracks; the leaving export works in the same scratch), plus max_tracks bytes once (the all-zero mask of
 *   mld_tracklets_step_lanes_device) and 16 * 96 * n_seq bytes of pinned host memory.
 *   Returns NULL on failure with the reason in *status_out (optional) and the text in mld_tracks_last_error(NULL).
 *   Destroy the store before its context.
 *
 * mld_tracks_begin_device: ids[s] = n_tracks[s] int32 ids (`int id = tracklet.id`, :29; every int32 value is an id).
 *   is_new_out[s][i] = 1 where ids[s][i] was not in the last committed frame of sequence s; is_new_out == NULL: the
 *   masks go to buffers of the store (what mld_tracklets_step_device uses).  n_tracks[s] <= max_tracks, 0 allowed.
 *   Ids must be unique within a sequence and frame: the reference's behaviour on a repeated id is an accident of
 *   std::map::emplace; here one occurrence is stored (which one is unspecified), the others are counted
 *   (mld_tracks_counts [5]) and export the stored occurrence's history.  A frame begun twice is begun afresh.
 *
 * mld_tracks_commit_device: per sequence the arrays of mld_tracklets_depths_device, d_cur / d_last being its outputs.
 *   A track that is not new gets ((int)u_new, (int)v_new, d_cur) pushed to the front; a new one is created with
 *   ((int)u_old, (int)v_old, d_last) and then gets the same push (length 2); u_old / v_old / d_last are read only there.
 *   Every track of the previous frame that is absent from this one is erased: after a commit the live set is exactly
 *   this frame's ids.  Coordinates are truncated as the reference's std::pair<int, int> does.
 *
 * mld_tracks_export_device: per sequence, for the tracks of the last committed frame in that frame's order:
 *   len_out[s][i] = stored entries of track i; fp_out[s] = n_tracks x max_history x 3 float32 (u, v, d), newest first,
 *   u / v the float of the stored integer (:237-238).  Entries at or beyond the length are NOT written (fixed stride: no
 *   callee resize, no prefix sum).  Either table may be NULL.
 *
 * mld_tracks_export_packed_device: the tracks of mld_tracks_export_device (last committed frame, that frame's order)
 *   without the holes.  offsets_out[s] (required) = n_tracks[s] + 1 int64: offsets[i] = the sum of the stored lengths of
 *   tracks 0 .. i-1, offsets[n] = the entries of the sequence; len_out[i] of the fixed-stride export is
 *   offsets[i+1] - offsets[i].  fp_out[s] = capacity[s] x 3 float32: entry e of track i (newest first, (u, v, d)) at
 *   position offsets[i] + e - bit for bit the concatenation over i of fp[i, :len[i]] of the fixed-stride export, a
 *   repeated id's history included.  The fp_out table may be NULL (offsets only); with it `capacity` is required,
 *   capacity[s] >= 0.  Positions >= capacity[s] are not written and nothing at or beyond min(offsets[n], capacity[s]) is
 *   touched; the offsets are complete all the same, so offsets[n] > capacity[s] tells a truncated sequence.
 *   capacity[s] = n_tracks[s] * max_history never truncates.  A sequence without tracks needs no arrays and gets nothing
 *   written; a capacity of 0 needs no fp_out[s].  Any other null array of a sequence with tracks is refused.  Asynchronous, no synchronisation, no host read of device data, nothing allocated per call.
 *
 * mld_tracks_export_leaving_device: what the commit of the BEGUN frame removes from the store, read between
 *   mld_tracks_begin_device and mld_tracks_commit_device (read-only; any number of calls, the commit is not affected).
 *   Per sequence s the stored tracks of the last committed frame are walked in that frame's (message) order;
 *   occurrences of a repeated id that lost are skipped, the stored occurrence stands for them.
 *   DEVIATION (order): the reference iterates its std::map, i.e. by ascending id (TidyUpTracklets :171-193); here both
 *   streams come in the committed frame's order.
 *   Ended tracks - tracks the begun frame's look-up did not find, which the commit erases: ids_out[s][k] = the id,
 *   offsets_out[s][k] = the sum of the stored lengths of the ended tracks in front of track k (int64), fp_out[s] = their
 *   entries back to back, (u, v, d) float32, newest first - per track the layout and the bits
 *   mld_tracks_export_packed_device writes for the same track.
 *   Spilled entries - for every track that continues with max_history stored entries, the oldest one, which the
 *   commit's push overwrites: spill_ids_out[s][k] = the id, spill_fp_out[s][3 * k ..] = the entry.  Tracks shorter than
 *   max_history spill nothing.  With both streams a consumer that appends the spilled entries to a track's tail and
 *   closes the track when it ends holds every track once and complete: the reference's unbounded deque at the moment
 *   TidyUpTracklets erases it (the max_history DEVIATION of mld_tracks_create loses nothing for such a consumer).
 *   flush (host, n_seq flags; NULL: none): a flagged sequence treats every stored track as ended, whatever the marks
 *   say, and spills nothing - the end of a recording, or a lane about to be restarted or reset.  When every sequence is
 *   flagged no begun frame is needed; otherwise a call without one returns MLD_ERR_NOT_INITIALIZED (a begin abandoned by
 *   an import counts as none).
 *   Capacities (host, n_seq each, >= 0): track_capacity[s] tracks in ids_out[s] and track_capacity[s] + 1 entries in
 *   offsets_out[s]; entry_capacity[s] entries in fp_out[s]; spill_capacity[s] entries in spill_ids_out[s] and
 *   spill_fp_out[s].  With w = min(n_ended, track_capacity[s]): ids_out[s][0 .. w-1] and offsets_out[s][0 .. w] are
 *   written (offsets[w] closes track w - 1; with track_capacity[s] == 0 nothing of either), entries at positions below
 *   min(n_ended_entries, entry_capacity[s]) whichever track they belong to, spills below min(n_spilled,
 *   spill_capacity[s]); nothing at or beyond these is touched.  n_committed, n_committed * max_history and n_committed -
 *   the track count of the last committed frame, which the host knows - never truncate.
 *   record_out_dev: n_seq mld_leaving_record in device memory, 8-byte aligned; every record is written completely by
 *   every call and its counts are complete, so n_ended > track_capacity[s] (and so on) tells a truncated sequence.  A
 *   sequence without committed tracks gets a record of zeros, needs no arrays and gets nothing else written.
 *   MLD_ERR_INVALID_ARG with "mld_tracks_export_leaving_device: <argument>" for a null table (all but flush are
 *   required), a null array of a sequence with committed tracks whose capacity is > 0, a negative capacity, an array
 *   that is not aligned to its element (offsets_out and record_out_dev: 8 bytes, the others 4); everything is checked
 *   before anything is queued.  Asynchronous, no synchronisation, no host read of device data, nothing allocated per
 *   call, no atomics (both streams are deterministic): three launches behind the descriptor upload, in the scratch of
 *   the packed export.
 *
 * mld_tracks_set_leaving_sink: the output arguments of mld_tracks_export_leaving_device for the NEXT
 *   mld_tracklets_step_device / mld_tracklets_step_lanes_device on the store, whose begin and commit lie inside one call.
 *   The tables are copied; the device arrays must stay valid until that step has run.  That step writes every
 *   sequence's record and streams in exactly one of two passes: a restarting sequence is flushed BEFORE it is emptied,
 *   every other sequence is exported by the marks AFTER the step's look-up.  The sink is then disarmed; a step that is
 *   refused before its look-up writes nothing and leaves it armed; a step that fails later has consumed it.  Checks as
 *   above, except that an array may be null only where its capacity is 0 (the step's track counts are not known yet).
 *   All arguments NULL disarms.  Without a sink a step queues exactly the launches it queues without this function.
 *
 * mld_tracks_import_packed_device: per sequence s with select[s] != 0 (select: host, n_seq flags; NULL: every sequence)
 *   the committed frame is replaced by the n_tracks[s] given tracks in the given (message) order: track i has id
 *   ids[s][i] and the entries fp[s][3 * (offsets[s][i] + e) ..], e < L = offsets[s][i+1] - offsets[s][i], newest first -
 *   the layout mld_tracks_export_packed_device writes (n + 1 int64 offsets, (u, v, d) float32 entries; device arrays, the
 *   tables of n_seq pointers / counts on the host).  Entries are stored bit for bit (no truncation to int: the caller
 *   hands in what an export produced), so that both exports and the counts of the store equal the source's and the
 *   frames that follow equal an uninterrupted run; the source may have another max_tracks / max_history, context or GPU.
 *   Sequences with select[s] == 0 are not touched in any way and their table entries may be NULL.  n_tracks[s] == 0
 *   empties the sequence (its arrays may be NULL).
 *   DEVIATIONS and bounds: L > max_history keeps the newest max_history entries (the cap of mld_tracks_create).
 *   n_entries[s] (host) = the entries fp[s] holds: offsets are clamped to [0, n_entries[s]] on the device, a decreasing pair
 *   gives length 0, nothing at or beyond n_entries[s] is read; a track of length 0 is stored with length 0 and the next
 *   commit pushes onto it.  offsets[s] always holds n_tracks[s] + 1 entries.  A repeated id follows the rule of
 *   mld_tracks_commit_device: one occurrence is stored (which one is unspecified), the others are counted and export the
 *   stored occurrence's history.  mld_tracks_counts of an imported sequence: [1] = tracks stored by the import, [2] = 0,
 *   [0] = [1] + [2], [3] / [4] over the stored entries as always, [5] = repeated ids.  A begun, uncommitted frame is
 *   abandoned for ALL sequences, as a second begin abandons it (the frame a failed step left behind included): a commit
 *   without a new begin returns MLD_ERR_NOT_INITIALIZED.  n_tracks[s] > max_tracks returns MLD_ERR_CAPACITY; a null table,
 *   a null array of a selected sequence with tracks (fp[s] only where n_entries[s] > 0), a negative count or n_entries
 *   MLD_ERR_INVALID_ARG; everything is checked before anything is queued or any host state changes.  Asynchronous, no
 *   synchronisation, no host read of device data, nothing allocated per call; the ids are read by this call only.  Two
 *   launches behind the descriptor upload, flat over the selected sequences: the reset (table cleared, row pool as created)
 *   and insert + fill.
 *
 * mld_tracks_reset_device: the import of no tracks into the selected sequences (select == NULL: all): one launch.
 *
 * mld_tracks_counts: counts_out = n_seq x 6 int64 of the last committed frame: [0] live tracks, [1] created this frame,
 *   [2] updated this frame, [3] stored features with d >= 0, [4] the other stored features, [5] repeated ids.
 *
 * mld_tracklets_step_device: arguments and bank convention as mld_tracklets_depths_device, with ids in place of is_new;
 *   `tr` must have been created on `ctx` with the same n_seq.  The caller supplies feature_points[1] (u_old / v_old) for
 *   every track; it is read only where the track turns out to be new.  d_last_out is written only there.  No
 *   synchronisation, no host read of device data.
 *
 * mld_tracklets_step_lanes_device: mld_tracklets_step_device with have_last[s] per sequence (host, n_seq flags, as
 *   mld_tracklets_depths_lanes_device) and restart (host, n_seq flags; NULL: none).  restart[s] != 0 is the construction
 *   of a new TrackletDepthModule for sequence s: its store is emptied ahead of the look-up (mld_tracks_reset_device of the
 *   restarting sequences: one more launch, only when there is one), have_last[s] counts as 0, every id of s is new - ids
 *   the sequence held a frame ago included - and its d_last is -1 (tracklet_depth_module.cpp:93-96).  With restart == NULL
 *   and equal flags the launches and results are those of mld_tracklets_step_device.  A step with mixed flags makes the
 *   same ONE launch set of the depth call with have_last = 1 and hands it an all-zero mask for the sequences without a
 *   previous frame, so that none of their previous features is evaluated; one more launch then writes their new tracks'
 *   d_last = -1 / MLD_Unspecified.  The previous-bank slots are checked as stated at mld_tracklets_depths_lanes_device.  What the begin refuses is refused
 *   before a sequence is emptied; a depth call that fails afterwards leaves the restarted sequences empty.
 */
typedef struct mld_tracks mld_tracks;
mld_tracks* mld_tracks_create(mld_ctx* ctx, int n_seq, int64_t max_tracks, int max_history, int* status_out);
void mld_tracks_destroy(mld_tracks* tr);
const char* mld_tracks_last_error(const mld_tracks* tr);
int mld_tracks_begin_device(mld_tracks* tr, const int32_t* const* ids, const int64_t* n_tracks, uint8_t* const* is_new_out);
int mld_tracks_commit_device(mld_tracks* tr, const float* const* u_new, const float* const* v_new, const float* const* u_old,
                             const float* const* v_old, const float* const* d_cur, const float* const* d_last);
int mld_tracks_export_device(mld_tracks* tr, float* const* fp_out, int32_t* const* len_out);
int mld_tracks_export_packed_device(mld_tracks* tr, float* const* fp_out, const int64_t* capacity,
                                    int64_t* const* offsets_out);
int mld_tracks_import_packed_device(mld_tracks* tr, const uint8_t* select, const int32_t* const* ids, const int64_t* n_tracks,
                                    const int64_t* const* offsets, const float* const* fp, const int64_t* n_entries);
int mld_tracks_reset_device(mld_tracks* tr, const uint8_t* select);
typedef struct mld_leaving_record {
    int64_t n_ended;          /* stored tracks of the committed frame that end */
    int64_t n_ended_entries;  /* their entries */
    int64_t n_spilled;        /* continuing tracks whose oldest entry is overwritten */
    int64_t reserved;         /* 0 */
} mld_leaving_record;         /* 32 bytes */
int mld_tracks_export_leaving_device(mld_tracks* tr, const uint8_t* flush, int32_t* const* ids_out, int64_t* const* offsets_out,
                                     float* const* fp_out, int32_t* const* spill_ids_out, float* const* spill_fp_out,
                                     const int64_t* track_capacity, const int64_t* entry_capacity, const int64_t* spill_capacity,
                                     void* record_out_dev);
int mld_tracks_set_leaving_sink(mld_tracks* tr, int32_t* const* ids_out, int64_t* const* offsets_out, float* const* fp_out,
                                int32_t* const* spill_ids_out, float* const* spill_fp_out, const int64_t* track_capacity,
                                const int64_t* entry_capacity, const int64_t* spill_capacity, void* record_out_dev);
int mld_tracks_counts(mld_tracks* tr, int64_t* counts_out);
int mld_tracklets_step_device(mld_ctx* ctx, mld_tracks* tr, int bank_cur, int have_last, const int32_t* const* ids,
                              const float* const* u_new, const float* const* v_new, const float* const* u_old,
                              const float* const* v_old, const int64_t* n_tracks, float* const* d_cur_out,
                              float* const* d_last_out, int32_t* const* type_cur_out, int32_t* const* type_last_out);
int mld_tracklets_step_lanes_device(mld_ctx* ctx, mld_tracks* tr, int bank_cur, const uint8_t* have_last, const uint8_t* restart,
                                    const int32_t* const* ids, const float* const* u_new, const float* const* v_new,
                                    const float* const* u_old, const float* const* v_old, const int64_t* n_tracks,
                                    float* const* d_cur_out, float* const* d_last_out, int32_t* const* type_cur_out,
                                    int32_t* const* type_last_out);

/*
 * Per-track semantic labels for a batch — matches_conversion_ros_tool's `semantic_labels` node, assignLabels
 * (src/semantic_labels/semantic_labels.cpp:50-72), which the reference's launch files run directly behind
 * tracklets_depth: for every track, the most frequent label of a mono8 label image in a window around the newest
 * feature point goes into TrackletWithOutlierFlag.label.  n_seq independent sequences per call, every array in GPU
 * memory.  (There is no host-pointer, one-frame form: see INTEGRATION.md.)
 *
 * Per track, with p = ((int)u, (int)v) - C++ truncation toward zero, -0.7 -> 0 - and INTEGER roi_width / 2,
 * roi_height / 2 (:56-60):
 *   columns [max(0, p.x - roi_width / 2),  min(cols, p.x + roi_width / 2))
 *   rows    [max(0, p.y - roi_height / 2), min(rows, p.y + roi_height / 2))
 * The window is 2 * (roi_width / 2) x 2 * (roi_height / 2) pixels, offset toward the upper left: the default roi 5 x 5
 * counts 4 x 4 pixels, columns p.x - 2 .. p.x + 1.  This is the reference's arithmetic and is kept.  The label is the
 * uchar value with the highest count in the window.
 *
 * Where the reference is undefined, this is defined:
 *   DEVIATION (ties): the reference takes std::max_element over a std::unordered_map, so among equally frequent labels
 *     the library's bucket order decides.  Here the SMALLEST label value among the most frequent wins.
 *   DEVIATION (empty window): roi_width / 2 == 0 or roi_height / 2 == 0, or a point so far outside the image that
 *     min >= max - OpenCV asserts on start > end and the reference dereferences end() on start == end.  Here the label
 *     is -2, the value matches_msg_conversions_ros/convert.hpp:53,97 gives every track before this node runs.
 *   DEVIATION (u or v not convertible): NaN, +-inf and values beyond the range of int are undefined behaviour in the
 *     reference's float -> int conversion.  Here they are an empty window (-2).  Everything else behaves as if computed
 *     in exact integer arithmetic: p +- roi / 2 does not overflow for any finite float and any roi >= 0.
 * Where none of the three applies the answer is unique and is the reference's.
 *
 * mld_labels_create: an object bound to `ctx` for calls of n_seq (1 .. 65536) sequences.  It owns 48 * n_seq bytes of
 *   device memory and 16 * 48 * n_seq bytes of pinned host memory (the descriptor ring); nothing is allocated per call.
 *   The size is checked before the context is looked at.  Returns NULL on failure with the reason in *status_out
 *   (optional) and the text in mld_labels_last_error(NULL).  Destroy the object before its context.
 *
 * mld_labels_assign_device: tables of n_seq entries.
 *   label_image_dev[s]  the image of sequence s: rows x cols uint8, row_stride_bytes >= cols between rows; neither the
 *                       base nor the stride needs any alignment.  One geometry for all sequences; rows, cols >= 1,
 *                       rows * cols < 2^31.
 *   roi_width, roi_height  >= 0, no upper limit (the window is clipped to the image).
 *   u[s], v[s]          n_tracks[s] float32 each: the newest feature of every track in the frame's order - the arrays
 *                       handed to mld_tracklets_step_device as u_new / v_new.  (The store keeps (float)(int)u, and
 *                       truncating that again gives the same pixel: labels of the raw features and of an exported
 *                       history's entry 0 are equal.)
 *   n_tracks[s]         >= 0; a sequence without tracks needs no arrays.
 *   label_out[s][i]     int16 as TrackletWithOutlierFlag.label: 0 .. 255, or -2.
 *   votes_out           optional - the table or single entries may be NULL.  votes_out[s] = n_tracks[s] x 2 int32: the
 *                       winner's count and the number of pixels of the clipped window (0, 0 for an empty one), so that
 *                       a caller can discard weak majorities.
 *   Asynchronous on the context's stream: no synchronisation, no host read of device data.  The host tables are
 *   consumed before the call returns; the device arrays must stay valid until the work has run.  Like a context, the
 *   object serves one call at a time.  MLD_ERR_INVALID_ARG with a text naming the argument (mld_labels_last_error; of
 *   NULL for a null object) on: a null object, a null table other than votes_out, a null array of a sequence that has
 *   tracks, rows or cols < 1, row_stride_bytes < cols, a negative roi, a negative n_tracks.
 */
typedef struct mld_labels mld_labels;
mld_labels* mld_labels_create(mld_ctx* ctx, int n_seq, int* status_out);
void mld_labels_destroy(mld_labels* lb);
const char* mld_labels_last_error(const mld_labels* lb);
int mld_labels_assign_device(mld_labels* lb, const uint8_t* const* label_image_dev, int rows, int cols,
                             int row_stride_bytes, int roi_width, int roi_height, const float* const* u,
                             const float* const* v, const int64_t* n_tracks, int16_t* const* label_out,
                             int32_t* const* votes_out);

/*
 * Semantic ground planes for a batch — SemanticPlane::CalculateInliersPlane (RansacPlane.cpp:195-274) for n_seq
 * independent sequences in one call: the plane TrackletDepthModule::process builds from the label image of every frame
 * (tracklet_depth_module.cpp:269-284, labels 6..9) and hands, un-segmented, to CalculateDepth.  What
 * mld_estimate_semantic_plane_device does for one slot (four launches, one synchronisation, after the slot's cloud has
 * been projected) this does for all sequences with four launches and none - and BEFORE the projection: clouds and
 * images are read where they lie, no slot is involved, and the masks it writes are the mask_dev[s] arrays of
 * mld_set_clouds_planes_range_device, so that the plane rides in the pixel-map keys.
 *
 * mld_semantic_planes_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536)
 *   sequences of up to max_points (1 .. 8 388 607) points each.  camera (focal_length, principal_point_x / _y; width and
 *   height are not read: the bounds are the label image's) and T_cam_lidar are the reference's SemanticPlane::Camera -
 *   pass the values the context was created with.  All memory is allocated here, none per call:
 *     device  n_seq * (40 * ceil(max_points / 64) + 48) bytes   (moment sums per 64 points, descriptor, first plane)
 *     pinned  16 * 32 * n_seq bytes                             (the descriptor ring)
 *   The sizes are checked before the context is looked at.  Returns NULL on failure with the reason in *status_out
 *   (optional) and the text in mld_semantic_planes_last_error(NULL).  Destroy the object before its context.
 *
 * mld_semantic_planes_estimate_device: tables of n_seq entries.
 *   pts_dev[s], n[s]    the cloud of sequence s: n[s] records of stride_bytes (16 or 32, x y z first), 4-byte aligned.
 *                       0 <= n[s] <= max_points (beyond it: MLD_ERR_CAPACITY).
 *   label_image_dev[s]  rows x cols uint8, row_stride_bytes >= cols between rows, no alignment.  One geometry and one
 *                       label set for all sequences; ground_labels outside 0 .. 255 never match.
 *   inlier_threshold    as mld_estimate_semantic_plane.
 *   result_out_dev      DEVICE array of n_seq records (4-byte aligned).
 *   mask_out_dev[s]     ceil(n[s] / 32) uint32 words, 4-byte aligned: bit i of word i / 32 = point i is an inlier.  Every
 *                       word is written, the bits at and beyond n[s] are 0, nothing beyond the last word is touched.
 *   Per sequence the record and the mask are bit for bit what mld_estimate_semantic_plane_device computes on the same
 *   cloud (same projection arithmetic, same association of the float moment sums, same eigenvector routine).  Three
 *   candidates are no failure: the first plane is then the dummy prior (0, 0, 1, 0) (:241-242).
 *   A sequence with n[s] < 3 or fewer than 3 candidates - the reference's ExceptionPclInvalid (:224-227), which the
 *   caller of the reference answers with depths of -1 from its catch block (tracklet_depth_module.cpp:338-351) - gets
 *   status 1, coefficients 0, n_inliers 0 (n_candidates: what was found) and a mask of zeros; the other sequences are
 *   unaffected and the return code stays MLD_OK.  What to do with such a frame is the caller's business (skip its depths,
 *   or run it without a plane).  n[s] == 0 needs no cloud, image or mask array and gets its record only.
 *   Asynchronous on the context's stream: no synchronisation, no host read of device data.  The host tables are consumed
 *   before the call returns, so a caller may queue frames ahead; the device arrays must stay valid until the work has
 *   run.  Like a context, the object serves one call at a time.
 *   The coefficients are wanted on the HOST by mld_set_clouds_planes_range_device: a caller that feeds that entry point
 *   copies the 32 * n_seq bytes of records back and synchronises once per batch.  That round trip remains; taking the
 *   coefficients from device memory would be a change inside the context.
 *   MLD_ERR_INVALID_ARG with a text naming the argument (mld_semantic_planes_last_error; of NULL for a null object) on:
 *   a null object or table, a null array of a sequence with points, rows or cols < 1, row_stride_bytes < cols, n[s] < 0,
 *   a stride other than 16 or 32, n_labels < 0 or ground_labels NULL with n_labels > 0, a cloud or mask that is not
 *   4-byte aligned.
 */
typedef struct mld_semantic_plane_result {   /* 32 bytes */
    float   coeffs[4];      /* plane of the refit, LIDAR frame (RansacPlane.cpp:253,259) */
    int32_t n_candidates;   /* points whose projection hit a ground label (:198-221) */
    int32_t n_inliers;      /* points within inlier_threshold of the first fit (:252) */
    int32_t status;         /* 0 ok, 1 = ExceptionPclInvalid (:224-227) */
    int32_t reserved;       /* 0 */
} mld_semantic_plane_result;

typedef struct mld_semantic_planes mld_semantic_planes;
mld_semantic_planes* mld_semantic_planes_create(mld_ctx* ctx, int n_seq, int64_t max_points, const mld_camera* camera,
                                                const double T_cam_lidar[12], int* status_out);
void mld_semantic_planes_destroy(mld_semantic_planes* sp);
const char* mld_semantic_planes_last_error(const mld_semantic_planes* sp);
int mld_semantic_planes_estimate_device(mld_semantic_planes* sp, const void* const* pts_dev, const int64_t* n,
                                        int stride_bytes, const uint8_t* const* label_image_dev, int rows, int cols,
                                        int row_stride_bytes, const int32_t* ground_labels, int n_labels,
                                        double inlier_threshold, mld_semantic_plane_result* result_out_dev,
                                        uint32_t* const* mask_out_dev);

/*
 * RANSAC ground planes for a batch — RansacPlane::CalculateInliersPlane (RansacPlane.cpp:41-140) for n_seq independent
 * sequences in one call: the plane of a frame that comes WITHOUT a label image, which DepthEstimator::setInputCloud
 * estimates by default (DepthEstimator.cpp:275-283).  The twin of mld_semantic_planes: what mld_estimate_ground_plane does
 * for one slot (after the slot's cloud has been projected, ending in a synchronisation) this does for all sequences with
 * up to three launches and no synchronisation - and BEFORE the projection: clouds are read where they lie, no slot is
 * involved (either bank of a two-bank slot layout is served alike), and the masks it writes are the mask_dev[s] arrays
 * of mld_set_clouds_planes_range_device.
 *
 * mld_ransac_planes_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences
 *   of up to max_points (1 .. 8 388 607) points each.  `params` is copied; of it only the fields the estimator reads are
 *   used: ransac_plane_distance_treshold, ransac_plane_min_z / _max_z (the z pass-through is on when min_z > -1001, as
 *   for mld_estimate_ground_plane), ransac_plane_max_iterations (0 .. 2^31 - 2), ransac_plane_probability,
 *   ransac_plane_use_refinement, ransac_plane_refinement_treshold.  All memory is allocated here, none per call:
 *     device  n_seq * (8 * ceil(max_points / 64) + 4 * ceil(max_points / 1024) + 28) bytes
 *             (pass-through: candidate mask per 64 points, candidate count per 1024 points; descriptor)
 *     pinned  16 * 24 * n_seq bytes   (the descriptor ring)
 *   max_points bounds that scratch and nothing else: there is no size of cloud at which a call takes another, slower or
 *   synchronising, path.  The sizes are checked before the context is looked at, then the context, then params.  Returns
 *   NULL on failure with the reason in *status_out (optional) and the text in mld_ransac_planes_last_error(NULL).
 *   Destroy the object before its context.
 *
 * mld_ransac_planes_estimate_device: HOST tables of n_seq entries.
 *   pts_dev[s], n[s]    the cloud of sequence s: n[s] records of stride_bytes (16 or 32, x y z first), 4-byte aligned.
 *                       0 <= n[s] <= max_points (beyond it: MLD_ERR_CAPACITY).
 *   seeds[s]            fixes the random draws of sequence s (the reference's pcl::RandomSample is time-seeded).
 *   result_out_dev      DEVICE array of n_seq records (4-byte aligned).
 *   mask_out_dev[s]     ceil(n[s] / 32) uint32 words, 4-byte aligned: bit i of word i / 32 = point i is an inlier.  Every
 *                       word is written, the bits at and beyond n[s] are 0, nothing beyond the last word is touched.
 *   Parity contract: per sequence the record and the mask are bit for bit what mld_estimate_ground_plane leaves on a slot
 *   that holds that cloud, with that seed - coefficients, the inlier set as mld_get_ground_plane_inliers lists it, and
 *   `iterations` as mld_calculate_depth_frame_estimate reports it (mld_plane_result.iterations).  Two properties of that
 *   path are kept with it: the inliers come from the (at most 6000) sampled points only, and a cloud in which no draw
 *   gives a plane within 10 degrees of the z axis adopts its first draw with 0 inliers (status 0).
 *   A sequence with n[s] < 3, fewer than three candidates of the pass-through or no model at all (every draw degenerate,
 *   e.g. a cloud of NaN) - GroundPlane::ExceptionPclInvalid - gets status 1, coefficients 0, n_inliers 0, iterations 0
 *   (n_candidates: what was found) and a mask of zeros; the other sequences are unaffected and the return code stays
 *   MLD_OK.  What to do with such a frame is the caller's business.  n[s] == 0 needs no cloud or mask array and gets its
 *   record only.
 *   Asynchronous on the context's stream: no synchronisation, no host read of device data.  The host tables are consumed
 *   before the call returns, so a caller may queue frames ahead; the device arrays must stay valid until the work has
 *   run.  Like a context, the object serves one call at a time.  As for mld_semantic_planes, a caller that feeds
 *   mld_set_clouds_planes_range_device copies the 32 * n_seq bytes of records back and synchronises once per batch.
 *   MLD_ERR_INVALID_ARG with a text naming the argument (mld_ransac_planes_last_error; of NULL for a null object) on: a
 *   null object or table, a null array of a sequence with points, n[s] < 0, a stride other than 16 or 32, a cloud or
 *   mask that is not 4-byte aligned.
 */
typedef struct mld_ransac_plane_result {   /* 32 bytes */
    float   coeffs[4];     /* LIDAR frame; what mld_estimate_ground_plane returns */
    int32_t n_inliers;     /* set bits of the mask */
    int32_t iterations;    /* iterations PCL's stopping rule counted (mld_plane_result.iterations) */
    int32_t status;        /* 0 ok, 1 = GroundPlane::ExceptionPclInvalid */
    int32_t n_candidates;  /* points that passed the z pass-through (n when it is off) */
} mld_ransac_plane_result;

typedef struct mld_ransac_planes mld_ransac_planes;
mld_ransac_planes* mld_ransac_planes_create(mld_ctx* ctx, int n_seq, int64_t max_points, const mld_params* params,
                                            int* status_out);
void mld_ransac_planes_destroy(mld_ransac_planes* rp);
const char* mld_ransac_planes_last_error(const mld_ransac_planes* rp);
int mld_ransac_planes_estimate_device(mld_ransac_planes* rp, const void* const* pts_dev, const int64_t* n, int stride_bytes,
                                      const uint32_t* seeds, mld_ransac_plane_result* result_out_dev,
                                      uint32_t* const* mask_out_dev);

/*
 * Projected clouds of a batch — the frame's PointcloudData (PointcloudData.h:13-68; DepthEstimator.cpp:155-218) for n_seq
 * independent sequences in one call: the visible list (getPointsCloudImageCs), _pointIndex, getPointDepthCamVisible, the
 * camera-frame cloud (getCloudCameraCs) and the reference-format pixel map _img_points_lidar (NeighborFinderPixel.cpp:
 * 38-55) - what the ROS layer's PublishImageProjectionCloud and PublishPointCloudCameraCs read.  What the debug / parity
 * getters below do for one slot (device memory allocated per slot, a synchronisation and a copy to the host per getter)
 * this does for all sequences with up to four launches, into DEVICE arrays of the caller, with no synchronisation: clouds
 * are read where they lie, no slot is involved.
 *
 * mld_projected_clouds_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences
 *   of up to max_points (1 .. 8 388 607) points each.  Of `camera` the width, height, focal length and principal point are
 *   read, and T_cam_lidar (row-major 3x4): pass the values the context was created with.  All memory is allocated here,
 *   none per call:
 *     device  n_seq * (8 * ceil(max_points / 64) + 4 * ceil(max_points / 1024) + 60) bytes
 *             (visibility mask per 64 points, visible count per 1024 points; descriptor)
 *     pinned  16 * 56 * n_seq bytes   (the descriptor ring)
 *   The sizes are checked before the context is looked at, then the context, then camera and T_cam_lidar (null; width or
 *   height < 1; width * height beyond 2^31 - 1).  Returns NULL on failure with the reason in *status_out (optional) and
 *   the text in mld_projected_clouds_last_error(NULL).  Destroy the object before its context.
 *
 * mld_projected_clouds_export_device: HOST tables of n_seq entries; every array they name is DEVICE memory, naturally
 *   aligned for its element type.
 *   pts_dev[s], n[s]    the cloud of sequence s: n[s] records of stride_bytes (16 or 32, x y z first), 4-byte aligned.
 *                       0 <= n[s] <= max_points (beyond it: MLD_ERR_CAPACITY).
 *   A point is VISIBLE iff its projection (u, v) - the exact f64 arithmetic of the depth path - satisfies 0 <= u <= W &&
 *   0 <= v <= H and 0 < u < W && 0 < v < H (DepthEstimator.cpp:184-207).  NaN and inf are not visible, z_cam == 0 is not;
 *   a point with z_cam < 0 may be.  Visible point r of a sequence is the r-th visible point in cloud order.
 *   n_visible_out_dev   required: DEVICE array of n_seq int64, [s] = Nvis of sequence s.  Always complete.
 *   uv_out[s]           2 x capacity[s] f64, column-major: (u, v) of visible point r at [2 r], [2 r + 1].
 *   index_out[s]        capacity[s] int32: the original index of visible point r (_pointIndex).
 *   depth_out           optional (the table, or single entries): capacity[s] f64, z_cam of visible point r
 *                       (getPointDepthCamVisible(r)).
 *   capacity[s]         >= 0.  Positions r >= capacity[s] are not written and nothing at or beyond min(Nvis, capacity[s])
 *                       is touched; n_visible_out_dev[s] > capacity[s] tells a truncated sequence.  capacity[s] = n[s]
 *                       never truncates; capacity[s] == 0 needs none of the three arrays.
 *   cam_out             optional (the table, or single entries): 3 x n[s] f64 column-major, the camera-frame coordinates
 *                       of ALL points (getCloudCameraCs) - not compacted, not subject to capacity.
 *   map_out             optional (the table, or single entries): W * H int32 at index x + y * W, the VISIBLE index of the
 *                       first visible point with z_cam > 0 whose ((int)u, (int)v) is that cell, else -1.  Every cell is
 *                       written on every call.  The values come from the complete ranks: the map of a truncated sequence
 *                       may hold values >= capacity[s].
 *   n[s] == 0 needs no arrays and gets n_visible 0, and its map (if given) all -1.
 *   Per sequence the outputs are bit for bit what mld_get_visible_count, mld_get_visible_image_points,
 *   mld_get_point_index, mld_get_cloud_camera_cs, mld_get_pixel_map and mld_get_point_depth_cam_visible give on a slot
 *   that holds that cloud (same transform and projection, operation for operation).
 *   Asynchronous on the context's stream: no synchronisation, no host read of device data, no runtime call per sequence.
 *   The host tables are consumed before the call returns, so a caller may queue frames ahead; the device arrays must stay
 *   valid until the work has run.  Like a context, the object serves one call at a time.
 *   MLD_ERR_INVALID_ARG with a text naming the argument (mld_projected_clouds_last_error; of NULL for a null object) on:
 *   a null object, a null table pts_dev, n, capacity, uv_out or index_out, a null n_visible_out_dev, a null cloud of a
 *   sequence with points, a null uv_out[s] or index_out[s] of a sequence with points and capacity, n[s] < 0,
 *   capacity[s] < 0, a stride other than 16 or 32, a cloud that is not 4-byte aligned.
 */
typedef struct mld_projected_clouds mld_projected_clouds;
mld_projected_clouds* mld_projected_clouds_create(mld_ctx* ctx, int n_seq, int64_t max_points, const mld_camera* camera,
                                                  const double T_cam_lidar[12], int* status_out);
void mld_projected_clouds_destroy(mld_projected_clouds* pc);
const char* mld_projected_clouds_last_error(const mld_projected_clouds* pc);
int mld_projected_clouds_export_device(mld_projected_clouds* pc, const void* const* pts_dev, const int64_t* n,
                                       int stride_bytes, const int64_t* capacity, int64_t* n_visible_out_dev,
                                       double* const* uv_out, int32_t* const* index_out, double* const* depth_out,
                                       double* const* cam_out, int32_t* const* map_out);

/*
 * Depth reports of a batch — the two per-frame products of the reference's ROS node (tracklets_depth_ros_tool,
 * tracklet_depth_interface.cpp:171-297) besides tracklets, camera-frame cloud and image projection, for n_seq independent
 * sequences in one call:
 *   the depth-calculation statistics  getDepthCalcStats (DepthEstimator.cpp:400-402), filled by LogDepthCalcStats
 *                                     (:1039-1090), published by PublishDepthCalcStats: one mld_depth_report per sequence
 *   the interpolated cloud            getCloudInterpolated (:339-341), published by PublishPointCloudInterpolated: the
 *                                     intersection point of the viewing ray with the local plane, one per feature with a
 *                                     depth
 * What mld_result_histogram does for one resultType array in host memory, and the host shim's getCloudInterpolated from the
 * debug vectors of a host-input call, this does for all sequences with at most three launches, from DEVICE arrays into
 * DEVICE arrays of the caller, with no synchronisation.
 *
 * mld_depth_report (192 bytes, 8-byte aligned):
 *   counts[t]       features of DepthResultType t, as mld_result_histogram
 *   other           features whose type lies outside [0, MLD_RESULT_TYPE_COUNT): dropped by mld_result_histogram, counted
 *                   here
 *   point_count     n_features[s] - DepthCalculationStatistics::SetPointCount(featuresCount) (DepthEstimator.cpp:484)
 *   n_interpolated  features with depth >= 0
 *
 * mld_depth_reports_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences
 *   of up to max_features (1 .. 16 777 216) features each.  Of `camera` the focal length and the principal point are
 *   read: pass the values the context was created with.  All memory is allocated here, none per call:
 *     device  n_seq * (8 * ceil(max_features / 64) + 92 * ceil(max_features / 1024) + 60) bytes
 *             (validity mask per 64 features; valid count and 22-bin type histogram per 1024 features; descriptor)
 *     pinned  16 * 56 * n_seq bytes   (the descriptor ring)
 *   The sizes are checked before the context is looked at, then the context, then the camera (null; focal_length not
 *   finite or 0).  Returns NULL on failure with the reason in *status_out (optional) and the text in
 *   mld_depth_reports_last_error(NULL).  Destroy the object before its context.
 *
 * mld_depth_reports_collect_device (DepthEstimator layer) and mld_depth_reports_collect_tracks_device (tracklet layer):
 *   HOST tables of n_seq entries; every array they name is DEVICE memory, naturally aligned for its element type.
 *   n_features[s]       0 <= n_features[s] <= max_features (beyond it: MLD_ERR_CAPACITY).
 *   collect_device      the arrays of mld_calculate_depths_device: uv[s] 2 x n_features[s] f64 column-major ((u, v) of
 *                       feature i at [2 i], [2 i + 1]), depth[s] f64, type[s] int32.
 *   collect_tracks_device  the arrays of mld_tracklets_depths_device / mld_tracklets_step_device: u[s], v[s] (u_new,
 *                       v_new) and depth[s] (d_cur) f32, type[s] (type_cur) int32.  d = (double)depth and
 *                       u = (double)truncf(u), likewise v: the integer pixel the tracklet layer evaluates
 *                       (std::pair<int,int>).  It equals (double)(int)u wherever that conversion is defined, and is
 *                       defined for NaN, +-inf and values beyond int as well.  This form serves the CURRENT-frame
 *                       results (d_cur, type_cur): they are what the reference's statistics hold after process(),
 *                       because the current-frame CalculateDepth runs last and clears them.  d_last is written only for
 *                       new tracks and is not a valid input.
 *   type                the table, or single entries, may be NULL: counts and other of those sequences are 0;
 *                       point_count and n_interpolated are still filled.
 *   report_out_dev      required: ONE device array of n_seq records.  Every record is written completely on every call;
 *                       a sequence with 0 features gets an all-zero record (and needs no arrays).
 *   A feature is INTERPOLATED iff depth >= 0, whatever its type says: NaN is out, -0.0 and +inf are in (as in the host
 *   shim's getCloudInterpolated, host/monolidar_fusion/DepthEstimator.h).  Its point is, in f64 and operation for
 *   operation as there and in depth_estimator.py,
 *       x = (u - cu) / f * d,   y = (v - cv) / f * d,   z = d.
 *   The reference's own push into this cloud is commented out (DepthEstimator.cpp:1028-1034), so its cloud is always
 *   empty; as with the existing getters, this is what the member is documented to hold (DepthEstimator.h:328).
 *   points_out[s]       capacity[s] x 3 f64: the points of the interpolated features IN FEATURE ORDER, point r at [3 r],
 *                       [3 r + 1], [3 r + 2].
 *   feature_out[s]      optional (the table, or single entries): capacity[s] int32, the feature index point r came from -
 *                       with it a caller joins the points with track ids.
 *   The points_out table may be NULL: statistics only; capacity and feature_out are then ignored.  With points_out,
 *   capacity is required and capacity[s] >= 0.  Points of rank >= capacity[s] are not written and nothing at or beyond
 *   min(n_interpolated, capacity[s]) is touched; n_interpolated is always complete, so n_interpolated > capacity[s] tells
 *   a truncated sequence.  capacity[s] = n_features[s] never truncates; capacity[s] == 0 needs neither array.
 *   Asynchronous on the context's stream: no synchronisation, no host read of device data, no runtime call per sequence,
 *   nothing allocated per call.  The host tables are consumed before the call returns, so a caller may queue frames
 *   ahead; the device arrays must stay valid until the work has run.  Like a context, the object serves one call at a
 *   time.
 *   MLD_ERR_INVALID_ARG with a text naming the function and the argument (mld_depth_reports_last_error; "null object
 *   (dr)" of NULL for a null object) on: a null object, a null table uv / u / v / depth / n_features, a null
 *   report_out_dev, a null input array of a sequence with features, n_features[s] < 0, a null capacity table with
 *   points_out, capacity[s] < 0, a null points_out[s] where min(capacity[s], n_features[s]) > 0, a float64 array or
 *   report_out_dev that is not 8-byte aligned, a float32 or int32 array that is not 4-byte aligned.
 */
typedef struct mld_depth_report {
    int64_t counts[MLD_RESULT_TYPE_COUNT];
    int64_t other;
    int64_t point_count;
    int64_t n_interpolated;
} mld_depth_report;

typedef struct mld_depth_reports mld_depth_reports;
mld_depth_reports* mld_depth_reports_create(mld_ctx* ctx, int n_seq, int64_t max_features, const mld_camera* camera,
                                            int* status_out);
void mld_depth_reports_destroy(mld_depth_reports* dr);
const char* mld_depth_reports_last_error(const mld_depth_reports* dr);
int mld_depth_reports_collect_device(mld_depth_reports* dr, const double* const* uv, const double* const* depth,
                                     const int32_t* const* type, const int64_t* n_features, const int64_t* capacity,
                                     mld_depth_report* report_out_dev, double* const* points_out,
                                     int32_t* const* feature_out);
int mld_depth_reports_collect_tracks_device(mld_depth_reports* dr, const float* const* u, const float* const* v,
                                            const float* const* depth, const int32_t* const* type,
                                            const int64_t* n_features, const int64_t* capacity,
                                            mld_depth_report* report_out_dev, double* const* points_out,
                                            int32_t* const* feature_out);

/*
 * Ground-plane inliers of a batch — what the reference keeps on a frame's GroundPlane besides the coefficients, for n_seq
 * independent sequences in one call:
 *   the inlier indices       GroundPlane::getInlinersIndex (RansacPlane.h:109): ascending original indices
 *   the lidar-frame matrix   GroundPlane::getMatrixFromIndices (RansacPlane.cpp:142-151): the float x, y, z of the inliers
 *   the camera-frame cloud   DepthEstimator::getCloudRansacPlane (DepthEstimator.cpp:294-308,396-398): the inliers in the
 *                            camera frame, filtered by ransac_plane_use_camx_treshold / ransac_plane_treshold_camx
 * The input is the inlier bitmask mld_semantic_planes_estimate_device and mld_ransac_planes_estimate_device write and
 * mld_set_clouds_planes_range_device takes.  What mld_get_ground_plane_inliers and mld_get_ground_plane_cloud do for one
 * slot (a copy of the mask - and of the whole camera-frame cloud - to the host, a synchronisation and a loop over every
 * point on the CPU per getter) this does for all sequences with at most three launches, into DEVICE arrays of the caller,
 * with no synchronisation: clouds and masks are read where they lie, no slot is involved, and the plane needs not be
 * installed on one.
 *
 * mld_plane_inliers_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences
 *   of up to max_points (1 .. 8 388 607) points each.  Of `params` only ransac_plane_use_camx_treshold and
 *   ransac_plane_treshold_camx are read, and they are copied; T_cam_lidar (row-major 3x4): pass the values the context
 *   was created with.  All memory is allocated here, none per call:
 *     device  n_seq * (8 * ceil(max_points / 1024) + 56) bytes, and with the camx filter on
 *             n_seq * 8 * ceil(max_points / 64) bytes more
 *             (inlier and cloud count per 1024 points, descriptor; the filter's ballot per 64 points)
 *     pinned  16 * 48 * n_seq bytes   (the descriptor ring)
 *   The sizes are checked before the context is looked at, then the context, then params and T_cam_lidar.  Returns NULL on
 *   failure with the reason in *status_out (optional) and the text in mld_plane_inliers_last_error(NULL).  Destroy the
 *   object before its context.
 *
 * mld_plane_inliers_export_device: HOST tables of n_seq entries; every array they name is DEVICE memory.
 *   pts_dev[s], n[s]    the cloud of sequence s: n[s] records of stride_bytes (16 or 32, x y z first), 4-byte aligned.
 *                       0 <= n[s] <= max_points (beyond it: MLD_ERR_CAPACITY).
 *   mask_dev[s]         ceil(n[s] / 32) uint32 words, 4-byte aligned (8-byte alignment is not needed): bit i of word
 *                       i / 32 = point i is an inlier.  The bits at and beyond n[s] in the last word are IGNORED - a
 *                       caller's own mask may carry anything there - and nothing beyond the last word is read.
 *   Inlier r of a sequence is the r-th set bit in cloud order.  An inlier is IN THE CLOUD iff the filter is off or
 *   fabs(x_cam) <= ransac_plane_treshold_camx; NaN fails.  Cloud point r is the r-th such inlier in cloud order.
 *   counts_out_dev      required: ONE device array of n_seq records, 8-byte aligned.  Always complete, whatever the
 *                       capacities and whichever outputs are null.
 *   index_out[s]        capacity[s] int32: the original index of inlier r, ascending - bit for bit what
 *                       mld_get_ground_plane_inliers lists on a slot that holds that cloud and mask.
 *   lidar_out           optional (the table, or single entries): 3 x capacity[s] float32 column-major, the x, y, z of
 *                       inlier r at [3 r], [3 r + 1], [3 r + 2]: the float bits of the record, copied.
 *   cam_out             optional (the table, or single entries): 3 x capacity[s] float64 column-major, the camera-frame
 *                       coordinates of cloud point r - bit for bit what mld_get_ground_plane_cloud writes, and what the
 *                       cam_out rows of mld_projected_clouds_export_device hold at those indices (same transform,
 *                       operation for operation).
 *   capacity[s]         >= 0.  ONE capacity bounds each list by its own rank: the inlier rank for index_out and lidar_out,
 *                       the cloud rank for cam_out.  Positions r >= capacity[s] are not written and nothing at or beyond
 *                       min(count, capacity[s]) is touched; n_inliers > capacity[s] (n_cloud > capacity[s]) tells a
 *                       truncated sequence.  capacity[s] = n[s] never truncates; capacity[s] == 0 needs none of the three
 *                       arrays.
 *   n[s] == 0 needs no cloud, mask or output array and gets a zero record.
 *   Asynchronous on the context's stream: no synchronisation, no host read of device data, no runtime call per sequence,
 *   nothing allocated per call.  The host tables are consumed before the call returns, so a caller may queue frames
 *   ahead; the device arrays must stay valid until the work has run.  Like a context, the object serves one call at a
 *   time.
 *   MLD_ERR_INVALID_ARG with a text naming the function and the argument (mld_plane_inliers_last_error; "null object
 *   (pi)" of NULL for a null object) on: a null object, a null table pts_dev, n, mask_dev, capacity or index_out, a null
 *   counts_out_dev, a null cloud or mask of a sequence with points, a null index_out[s] where min(capacity[s], n[s]) > 0,
 *   n[s] < 0, capacity[s] < 0, a stride other than 16 or 32, a cloud, mask, index_out or lidar_out array that is not
 *   4-byte aligned, a cam_out array or counts_out_dev that is not 8-byte aligned.
 */
typedef struct mld_plane_inlier_counts {   /* 16 bytes */
    int64_t n_inliers;   /* set mask bits below n[s]                       (getInlinersIndex().size()) */
    int64_t n_cloud;     /* those that pass the camx filter; == n_inliers when the filter is off */
} mld_plane_inlier_counts;

typedef struct mld_plane_inliers mld_plane_inliers;
mld_plane_inliers* mld_plane_inliers_create(mld_ctx* ctx, int n_seq, int64_t max_points, const mld_params* params,
                                            const double T_cam_lidar[12], int* status_out);
void mld_plane_inliers_destroy(mld_plane_inliers* pi);
const char* mld_plane_inliers_last_error(const mld_plane_inliers* pi);
int mld_plane_inliers_export_device(mld_plane_inliers* pi, const void* const* pts_dev, const int64_t* n, int stride_bytes,
                                    const uint32_t* const* mask_dev, const int64_t* capacity,
                                    mld_plane_inlier_counts* counts_out_dev, int32_t* const* index_out,
                                    float* const* lidar_out, double* const* cam_out);

/*
 * Per-feature traces of a batch — why a feature got the depth it got, for n_seq independent sequences in one call:
 *   the triangle corners     getCloudTriangleCorners / ActivateDebugMode (DepthEstimator.cpp:348-350,
 *                            PlaneEstimationCalcMaxSpanningTriangle.cpp:20-35)
 *   the per-feature record   DepthCalcStatsSinglePoint (do_debug_singleFeatures, DepthCalcStatsSinglePoint.h:20-67): the
 *                            neighbours, the segmented points, the histogram borders and the plane
 * What mld_calculate_depth_debug does for one slot (features from the host, every feature through the wave-cooperative
 * depth kernel, nine corner coordinates back to the host) this does for all sequences with two launches, into DEVICE
 * arrays of the caller, with no synchronisation and without a frame slot.  It re-walks the STRUCTURAL part of the
 * per-feature path on the arrays mld_projected_clouds_export_device writes, plus (optionally) the plane that
 * mld_semantic_planes / mld_ransac_planes leave on the device, operation for operation as the depth path does; integers
 * and float bits of a record equal what that path worked with.  Stages traced:
 *   1. the 1.0 x 1.0 window (NeighborFinderPixel.cpp:60-95): half sizes and clamping in f64, (int) truncation of the
 *      bounds.  A non-finite u or v gives an empty window and sets MLD_TRACE_FLAG_NONFINITE_FEATURE.
 *      n_nb < radiusSearch_count_min (compared as unsigned): main_type 2, the road is not reached.
 *   2. the histogram segmentation (HistogramPointDepth.cpp:15-123) including its lastBinValue early return; with
 *      do_use_histogram_segmentation off every neighbour is kept.
 *   3. the corners: the farthest pair with strict '>' (the first pair in (i, j) order wins), the third corner (the last
 *      point is never one); with do_use_triangle_size_maximation off the first three points.  Then the planarity test, the
 *      viewing ray through Kinv with the flip, Hyperplane::Through with its degenerate fallback, the orthogonality test,
 *      the global and local thresholds and cut-behind-camera.  main_type / main_depth are the result of this main path.
 *   4. the road fallback, when the sequence has a plane, do_use_ransac_plane is on and main_type is neither 1 nor 2: the
 *      2.0 x 1.5 window, the f32 un-normalised point-to-plane distance after the f64 camera->lidar transform, the mask
 *      bit of the original index.  The road fit itself is NOT repeated.  road_state says where the path ended:
 *        MLD_TRACE_ROAD_FAR_NEIGHBOUR   a neighbour farther than ransac_plane_point_distance_treshold: the final type is
 *                                       main_type, the final depth -1; n_road_inl is 0 and no inlier list is written
 *                                       (the reference leaves at that neighbour)
 *        MLD_TRACE_ROAD_FEW_INLIERS     fewer than three inliers: the final type is main_type, the final depth -1
 *        MLD_TRACE_ROAD_FIT             the estimator ran: type and depth are whatever the depth call returned
 *        MLD_TRACE_ROAD_FEW_NEIGHBOURS  n_road < radiusSearch_count_min, evaluated as the reference evaluates it
 *                                       (DepthEstimator.cpp:585-586).  It cannot occur: the wide window contains the
 *                                       narrow one, whose count has passed the same test.
 *
 * mld_feature_traces_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences
 *   of up to max_features (1 .. 16 777 216) features each.  params, camera and T_cam_lidar (row-major 3x4) are copied:
 *   pass the values the context was created with.  All memory is allocated here, none per call:
 *     device  120 * n_seq bytes        (the descriptors)
 *     pinned  16 * 120 * n_seq bytes   (the descriptor ring)
 *   The sizes are checked before the context is looked at, then the context, then params, camera and T_cam_lidar (null),
 *   and then, still without a use of the context:
 *     MLD_ERR_UNSUPPORTED_MODE  do_use_PCA (the eigen-solve is a tolerance path, the trace promises equality)
 *     the refusals of mld_create for a parameter set, a camera and a transform, with its status codes
 *     MLD_ERR_CAPACITY          a wide window that can cover more than 1024 cells, counted as
 *                               min(W, floor(2 halfX2) + 2) * min(H, floor(2 halfY2) + 2) with halfX2 =
 *                               pixelarea_search_witdh * 0.5 * 2.0 and halfY2 = pixelarea_search_height * 0.5 * 1.5
 *                               (C0: 14 x 15 = 210)
 *   Returns NULL on failure with the reason in *status_out (optional) and the text in
 *   mld_feature_traces_last_error(NULL).  Destroy the object before its context.
 *
 * mld_feature_traces_collect_device (DepthEstimator layer: uv[s] 2 x n_features[s] f64 column-major) and
 * mld_feature_traces_collect_tracks_device (tracklet layer: u[s], v[s] f32; u = (double)truncf(u), likewise v, exactly as
 * mld_depth_reports_collect_tracks_device): HOST tables of n_seq entries, consumed before the call returns; every array
 * they name is DEVICE memory, naturally aligned for its element type (the records: 8 bytes).
 *   n_features[s]       0 <= n_features[s] <= max_features (beyond it: MLD_ERR_CAPACITY).  A sequence with 0 features
 *                       needs no arrays.
 *   map[s]              W * H int32, index x + y * W: the visible index, or -1
 *   index[s], index_len[s]   _pointIndex: the original index of visible point r, index_len[s] entries
 *   cam[s], n_points[s] 3 x n_points[s] f64 column-major, the camera-frame cloud
 *                       All three exactly as mld_projected_clouds_export_device wrote them for that cloud (pixel_map_out,
 *                       index_out with a capacity that did not truncate, cam_out); n_points[s], index_len[s] <= 8 388 607.
 *   coeffs, mask_dev    as mld_set_clouds_planes_range_device takes them (n_seq x 4 floats on the HOST; a host table of
 *                       device bitmasks of ceil(n_points[s] / 32) words), both or neither.  A NULL mask_dev[s]: sequence s
 *                       has no plane (the reference's ransacPlane == nullptr).
 *   trace_out[s]        n_features[s] records; every record is written completely on every call.
 *   nb_out, seg_out, road_out, road_inl_out   optional (the table, or single entries): list_capacity x n_features[s] int32
 *                       each, feature i's row at i * list_capacity.
 *                         nb_out        visible indices of the narrow window's neighbours, in the reference's row-major
 *                                       scan order
 *                         seg_out       positions into that list of the neighbours the segmentation kept
 *                         road_out      visible indices of the wide window's neighbours
 *                         road_inl_out  positions into that list of the plane inliers
 *                       The first min(count, list_capacity) entries of a row are written and nothing behind them is
 *                       touched; the counts of the record are always complete, so a truncated row shows.
 *   list_capacity       0 .. 1024; with 0 no list array is needed or written.
 *   Robustness: a map value other than -1 outside [0, index_len[s]) and an index value outside [0, n_points[s]) make the
 *   cell count as EMPTY and set MLD_TRACE_FLAG_BAD_INPUT on the features whose scanned windows met it; no read leaves the
 *   arrays as the host tables size them.
 *   Asynchronous on the context's stream: no synchronisation, no host read of device data, no runtime call per sequence,
 *   nothing allocated per call, at most two launches (the descriptor upload and k_feature_trace, one wavefront per
 *   feature).  The device arrays must stay valid until the work has run.  Like a context, the object serves one call at a
 *   time.
 *   MLD_ERR_INVALID_ARG with a text naming the function and the argument (mld_feature_traces_last_error; "null object
 *   (ft)" of NULL for a null object) on: a null object, a null table uv / u / v, n_features, map, index, index_len, cam,
 *   n_points or trace_out, a null uv / u / v, map or trace_out array of a sequence with features (index, cam: where
 *   index_len[s], n_points[s] > 0), a negative count, list_capacity outside 0 .. 1024, coeffs without mask_dev or the
 *   other way round, an int32 or float array that is not 4-byte aligned, an f64 array or trace_out that is not 8-byte
 *   aligned.
 */
enum { MLD_TRACE_ROAD_NOT_REACHED = 0, MLD_TRACE_ROAD_FEW_NEIGHBOURS = 1, MLD_TRACE_ROAD_FAR_NEIGHBOUR = 2,
       MLD_TRACE_ROAD_FEW_INLIERS = 3, MLD_TRACE_ROAD_FIT = 4 };
enum { MLD_TRACE_FLAG_BAD_INPUT = 1, MLD_TRACE_FLAG_NONFINITE_FEATURE = 2 };

typedef struct mld_feature_trace {      /* 184 bytes, 8-byte aligned */
    int32_t main_type;      /* DepthResultType at the end of the main path (DepthEstimator.cpp:509-577) */
    int32_t road_state;     /* MLD_TRACE_ROAD_* */
    int32_t n_nb, n_seg;    /* neighbours of the 1.0 x 1.0 window; those the segmentation kept (0 if it failed) */
    int32_t n_road, n_road_inl; /* neighbours of the 2.0 x 1.5 window; plane inliers among them */
    int32_t corner_pos[3];  /* positions into the segmented list, -1 without corners */
    int32_t corner_vis[3];  /* their visible indices, -1 */
    int32_t flags, pad_;
    double  main_depth;     /* depth at the end of the main path: -1 unless main_type == MLD_Success */
    double  hist_lower, hist_higher;  /* borders of the chosen bin (HistogramPointDepth.cpp:99-100), -1 without one */
    double  plane_n[3], plane_offset; /* Hyperplane::Through of the corners; NaN unless the plane was formed */
    double  corners[9];     /* camera-frame corner1, corner2, corner3 (getCloudTriangleCorners); NaN without corners */
} mld_feature_trace;

typedef struct mld_feature_traces mld_feature_traces;
mld_feature_traces* mld_feature_traces_create(mld_ctx* ctx, int n_seq, int64_t max_features, const mld_params* params,
                                              const mld_camera* camera, const double T_cam_lidar[12], int* status_out);
void mld_feature_traces_destroy(mld_feature_traces* ft);
const char* mld_feature_traces_last_error(const mld_feature_traces* ft);
int mld_feature_traces_collect_device(mld_feature_traces* ft, const double* const* uv, const int64_t* n_features,
                                      const int32_t* const* map, const int32_t* const* index, const int64_t* index_len,
                                      const double* const* cam, const int64_t* n_points, const float* coeffs,
                                      const uint32_t* const* mask_dev, int list_capacity, mld_feature_trace* const* trace_out,
                                      int32_t* const* nb_out, int32_t* const* seg_out, int32_t* const* road_out,
                                      int32_t* const* road_inl_out);
int mld_feature_traces_collect_tracks_device(mld_feature_traces* ft, const float* const* u, const float* const* v,
                                             const int64_t* n_features, const int32_t* const* map, const int32_t* const* index,
                                             const int64_t* index_len, const double* const* cam, const int64_t* n_points,
                                             const float* coeffs, const uint32_t* const* mask_dev, int list_capacity,
                                             mld_feature_trace* const* trace_out, int32_t* const* nb_out, int32_t* const* seg_out,
                                             int32_t* const* road_out, int32_t* const* road_inl_out);

/*
 * Coverage maps of a batch — where in the image a feature can get a depth, for n_seq independent sequences in one call.
 * Whether a feature at pixel (x, y) clears the neighbour test, and whether the road fallback can run for it, is decided
 * before any floating-point fit: it depends only on the pixel map, the inlier mask and the window rule of
 * NeighborFinderPixel::getNeighbors (NeighborFinderPixel.cpp:60-95, with DepthEstimator.cpp:680-681 and :782-830).  This
 * object evaluates that neighbour stage at EVERY integer pixel of every sequence, in GPU memory, and names the best pixel
 * per bucket of the image - the list a feature detector would use.  Exact integers throughout; no tolerance path.
 *
 * The pixel (x, y), 0 <= x < W, 0 <= y < H, stands for the feature ((double)x, (double)y), the coordinate the tracklet
 * layer passes.  The windows are those of mld_feature_traces stage 1 and stage 4: half sizes
 *   halfX = (double)pixelarea_search_witdh * 0.5 * (double)sx,  halfY = (double)pixelarea_search_height * 0.5 * (double)sy
 * with (sx, sy) = (1.0f, 1.0f) for the narrow and (2.0f, 1.5f) for the wide window, the edges clamped in f64 to [0, W - 1]
 * and [0, H - 1], the bounds truncated with (int), both bounds scanned inclusive.  Column bounds depend on x only and row
 * bounds on y only; both are evaluated by that rule and never as x +- const (the clamped borders and the truncation of a
 * non-integer half size - C0 wide: 6.75 - differ).
 *
 * Per-cell properties, from map[s], index[s], cam[s], coeffs and mask_dev[s] (the arrays
 * mld_feature_traces_collect_device takes):
 *   occupied  the map value is not -1
 *   inlier    occupied, and the mask bit of index[r] is set
 *   far       occupied, and the f32 un-normalised point-to-plane distance of T_lidar_cam * p_cam (f64 transform, then cast
 *             to f32) exceeds ransac_plane_point_distance_treshold: operation for operation MLD_TRACE_ROAD_FAR_NEIGHBOUR
 *   A map value other than -1 outside [0, index_len[s]) and an index value outside [0, n_points[s]) make the cell EMPTY and
 *   set MLD_COVERAGE_FLAG_BAD_INPUT in the sequence's record; no read leaves the arrays as the host tables size them.
 *   A sequence without a plane - mask_dev[s] NULL, or coeffs NULL, or do_use_ransac_plane off - has no inlier and no far
 *   cells, and bit 1 of reach is 0 everywhere.
 *
 * Per-pixel outputs, W * H uint8 each with index x + y * W; every table and every entry is optional; counts saturate at 255:
 *   nb_out        occupied cells of the narrow window: n_nb of mld_feature_trace
 *   road_out, road_inl_out, road_far_out   occupied, inlier and far cells of the wide window
 *   reach_out     bit 0: n_nb >= radiusSearch_count_min (compared as unsigned): a feature there is not type 2
 *                 bit 1: bit 0, the sequence has a plane, n_road >= radiusSearch_count_min, n_far == 0 and n_inl >= 3: the
 *                        road estimator can run if the main path does not succeed
 *                 with set_all_depths_to_zero both bits are 0
 * record_out_dev: n_seq records (DEVICE memory, 8-byte aligned), every one written completely on every call.
 * Bucket proposals (bucket_out non-NULL): the image is cut into ceil(W / bucket_w) x ceil(H / bucket_h) buckets in
 *   row-major order; bucket b gets the int32[3] entry (x, y, n_nb) at bucket_out[s] + 3 * b: the pixel of the bucket with
 *   bit 0 set and the largest n_nb (before saturation); on equal counts the smallest y wins, then the smallest x; a bucket
 *   without such a pixel gets (-1, -1, 0).  The first min(buckets, bucket_capacity[s]) entries are written and nothing
 *   behind them is touched; n_buckets of the record is complete.  bucket_out NULL: no buckets, bucket_w, bucket_h and
 *   bucket_capacity are not looked at and n_buckets is 0.
 *
 * mld_coverage_maps_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences.
 *   params, camera and T_cam_lidar (row-major 3x4) are copied: pass the values the context was created with.  All memory
 *   is allocated here, none per call; with WW = ceil(W / 64):
 *     device  112 * n_seq bytes                 (the descriptors)
 *             24 * WW * H * n_seq bytes         (three bit planes: a row is WW 64-bit words)
 *             16 * (ceil(WW * H / 16) + ceil(W / 256) * ceil(H / BR)) * n_seq bytes   (block partials of the record; BR =
 *                                               16 rows, 8 where the wide window can span more than 16 rows)
 *             2 * W * H * n_seq bytes           (bucket partials: the unsaturated n_nb of the pixels with bit 0)
 *     pinned  16 * 112 * n_seq bytes            (the descriptor ring)
 *   The size is checked before the context is looked at, then the context, then params, camera and T_cam_lidar (null),
 *   and then, still without a use of the context:
 *     the refusals of mld_create for a parameter set, an image size and a transform, with its status codes
 *     MLD_ERR_CAPACITY          a wide window that can span more than 64 columns or more than 64 rows, counted as
 *                               min(W, floor(2 halfX2) + 2) and min(H, floor(2 halfY2) + 2) (C0: 14 x 15): the part of a
 *                               window in a row lies in at most two words
 *     MLD_ERR_CAPACITY          n_seq sequences of an image that need more than 2^31 - 1 blocks
 *   Returns NULL on failure with the reason in *status_out (optional) and the text in
 *   mld_coverage_maps_last_error(NULL).  Destroy the object before its context.
 *
 * mld_coverage_maps_collect_device: HOST tables of n_seq entries, consumed before the call returns; every array they name
 * is DEVICE memory, naturally aligned for its element type.
 *   map[s]              W * H int32, index x + y * W: the visible index, or -1.  Every sequence has one.
 *   index[s], index_len[s], cam[s], n_points[s], coeffs, mask_dev   as mld_feature_traces_collect_device takes them
 *   bucket_w, bucket_h  1 .. 65535 each;  bucket_capacity[s] >= 0 entries of bucket_out[s] (NULL with capacity 0)
 *   Asynchronous on the context's stream: no synchronisation, no host read of device data, no runtime call per sequence,
 *   nothing allocated per call, no atomics, four launches: the descriptor upload, k_coverage_classify (cells into bit
 *   planes; the map and the index are read once, here), k_coverage_count (window counts, the maps, reach; every requested
 *   output is written once) and k_coverage_finish (the record from block partials, the buckets).  The device arrays must
 *   stay valid until the work has run.  Like a context, the object serves one call at a time.
 *   MLD_ERR_INVALID_ARG with a text naming the function and the argument (mld_coverage_maps_last_error; "null object
 *   (cm)" of NULL for a null object) on: a null object, a null table map, index, index_len, cam or n_points, a null or
 *   misaligned record_out_dev, coeffs without mask_dev or the other way round, with bucket_out a bucket_w or bucket_h
 *   outside 1 .. 65535 or a null table bucket_capacity, a negative count, a null map array (index, cam: where index_len[s],
 *   n_points[s] > 0; bucket_out[s]: where bucket_capacity[s] > 0), an int32 array that is not 4-byte aligned, an f64 array
 *   that is not 8-byte aligned.  MLD_ERR_CAPACITY on n_points[s] or index_len[s] beyond 8 388 607 and on buckets so small
 *   that the call needs more than 2^31 - 1 blocks.
 */
enum { MLD_COVERAGE_REACH_MAIN = 1, MLD_COVERAGE_REACH_ROAD = 2 };
enum { MLD_COVERAGE_FLAG_BAD_INPUT = 1, MLD_COVERAGE_FLAG_HAS_PLANE = 2 };

typedef struct mld_coverage_record {    /* 64 bytes, 8-byte aligned */
    int64_t n_reach;        /* pixels with bit 0 of reach */
    int64_t n_reach_road;   /* pixels with bit 1 of reach */
    int64_t n_occupied, n_inlier, n_far;  /* cells of the map */
    int32_t max_nb;         /* the largest n_nb of a pixel, before saturation */
    int32_t flags;          /* MLD_COVERAGE_FLAG_* */
    int32_t n_buckets;      /* ceil(W / bucket_w) * ceil(H / bucket_h) of the call; 0 without buckets */
    int32_t pad_[3];
} mld_coverage_record;

typedef struct mld_coverage_maps mld_coverage_maps;
mld_coverage_maps* mld_coverage_maps_create(mld_ctx* ctx, int n_seq, const mld_params* params, const mld_camera* camera,
                                            const double T_cam_lidar[12], int* status_out);
void mld_coverage_maps_destroy(mld_coverage_maps* cm);
const char* mld_coverage_maps_last_error(const mld_coverage_maps* cm);
int mld_coverage_maps_collect_device(mld_coverage_maps* cm, const int32_t* const* map, const int32_t* const* index,
                                     const int64_t* index_len, const double* const* cam, const int64_t* n_points,
                                     const float* coeffs, const uint32_t* const* mask_dev, uint8_t* const* nb_out,
                                     uint8_t* const* road_out, uint8_t* const* road_inl_out, uint8_t* const* road_far_out,
                                     uint8_t* const* reach_out, mld_coverage_record* record_out_dev, int bucket_w, int bucket_h,
                                     const int64_t* bucket_capacity, int32_t* const* bucket_out);

/*
 * Depth images of a batch — the depth path at every pixel of a grid over the camera image, for n_seq independent sequences
 * in one call: what a depth call answers for a feature, answered for every pixel, or every n-th pixel, in GPU memory.  No
 * frame slot, no uv array, no synchronisation.  Every grid pixel gets the full per-feature path (SURVEY.md 8(a), rows B1 to
 * B10): the narrow window by the f64 rule of mld_coverage_maps (never x +- const), the histogram segmentation with all its
 * early returns, the max-spanning triangle or the first three points, the planarity test, the viewing ray with its flip,
 * Hyperplane::Through with the orthogonality test, the global and local thresholds and cut-behind-camera; and the road
 * fallback: the wide window, the f32 far test after the f64 camera->lidar transform, the mask bit of the original index,
 * the M-estimator fit (its weighted sums taken about the list's first point), the `Normal` intersection, the thresholds,
 * type 16.  Types are the reference's, main-path depths are bit for bit the depth calls', road depths agree to the road
 * tolerance of the project (1e-4 m).
 *
 * Inputs: map[s], index[s], index_len[s], cam[s], n_points[s], coeffs and mask_dev as mld_coverage_maps_collect_device takes
 * them, with the same meaning and the same bad-input rule: a map value other than -1 outside [0, index_len[s]) and an index
 * value outside [0, n_points[s]) make the cell EMPTY and - when a window that is scanned meets the cell - set
 * MLD_DEPTH_IMAGE_FLAG_BAD_INPUT in the sequence's record; no read leaves the arrays as the host tables size them.  A
 * sequence without a plane - mask_dev[s] NULL, or coeffs NULL, or do_use_ransac_plane off - has no road fallback.
 *
 * Grid: grid pixel (i, j), 0 <= i < grid_w, 0 <= j < grid_h, stands for the feature ((double)(x0 + i * step_x),
 * (double)(y0 + j * step_y)); its outputs have the index i + j * grid_w.  The grid lies inside the image and the steps are
 * >= 1: otherwise MLD_ERR_INVALID_ARG with a text naming the argument.
 *
 * Outputs, grid_w * grid_h entries each; every table and every entry is optional; each one asked for is written exactly
 * once and nothing outside it is touched:
 *   type_out     uint8: the DepthResultType
 *   depth_out    f64 (8-byte aligned): the path's depth, -1 on every failure, as the depth calls return it
 *   depth32_out  f32 (4-byte aligned): (float) of that value, the precision FeaturePoint.d carries
 * record_out_dev: n_seq records (DEVICE memory, 8-byte aligned), every one written completely on every call.
 *
 * mld_depth_images_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences.
 *   params, camera and T_cam_lidar (row-major 3x4) are copied: pass the values the context was created with.  All memory
 *   is allocated here, none per call; with TILES = ceil(W / 64) * ceil(H / 16), the tiles of the full grid:
 *     device  120 * n_seq bytes                 (the descriptors)
 *             128 * TILES * n_seq bytes         (overflow words: four 64-bit words per wavefront, four wavefronts per tile)
 *             512 * TILES * n_seq bytes         (partial counts of the record: 32 int32 per wavefront)
 *     pinned  16 * 120 * n_seq bytes            (the descriptor ring)
 *   Judged in this order, the context LAST and nothing of it used before: the size; params, camera and T_cam_lidar (null:
 *   MLD_ERR_INVALID_ARG); then
 *     MLD_ERR_UNSUPPORTED_MODE  do_use_PCA (the eigen-solve is a tolerance path), plane_estimator_use_triangle_maximation
 *                               (the triangle road estimator is a rare path) and set_all_depths_to_zero (the depth calls
 *                               answer it without a kernel), in this order
 *     the refusals of mld_create for a parameter set, an image size, intrinsics and a transform, with its status codes
 *     MLD_ERR_CAPACITY          a wide window that can cover more than 1024 cells, counted as mld_feature_traces counts it
 *     MLD_ERR_CAPACITY          n_seq sequences of an image that need more than 2^31 - 1 blocks
 *     MLD_ERR_INVALID_ARG       a null context
 *   Returns NULL on failure with the reason in *status_out (optional) and the text in
 *   mld_depth_images_last_error(NULL).  Destroy the object before its context.
 *
 * mld_depth_images_render_device: HOST tables of n_seq entries, consumed before the call returns; every array they name is
 * DEVICE memory.  Asynchronous on the context's stream: no synchronisation, no host read of device data, no runtime call per
 *   sequence, nothing allocated per call, no atomics, four launches: the descriptor upload, k_depth_image_lane (one lane
 *   per grid pixel over tiles of 64 x 16 grid pixels whose map cells, halo included, are staged in LDS once; type-2 pixels
 *   leave on the count alone; lists of up to 32 entries per lane), k_depth_image_coop (one wavefront per pixel whose narrow
 *   list or whose list of road inliers is longer than 32 entries; lists up to the 1024-cell bound) and
 *   k_depth_image_finish (the record from per-wavefront partial counts).  Which route a pixel takes changes no output
 *   beyond the road tolerance and no type.  The device arrays must stay valid until the work has run.  Like a context, the
 *   object serves one call at a time.
 *   MLD_ERR_INVALID_ARG with a text naming the function and the argument (mld_depth_images_last_error; "null object (di)"
 *   of NULL for a null object) on: a null object, a null table map, index, index_len, cam or n_points, a null or
 *   misaligned record_out_dev, coeffs without mask_dev or the other way round, step_x or step_y below 1, grid_w or grid_h
 *   below 1, x0 or y0 outside the image, a last column or row outside the image, a negative count, a null map array
 *   (index, cam: where index_len[s], n_points[s] > 0), an int32 or f32 array that is not 4-byte aligned, an f64 array that is
 *   not 8-byte aligned.  MLD_ERR_CAPACITY on n_points[s] or index_len[s] beyond 8 388 607.
 * In libmld_hip_ab.so only, MLD_DEPTH_IMAGE_COOP=1 in the environment, read at create, sends every pixel that clears the
 * neighbour test through k_depth_image_coop.
 */
enum { MLD_DEPTH_IMAGE_FLAG_BAD_INPUT = 1, MLD_DEPTH_IMAGE_FLAG_HAS_PLANE = 2 };

typedef struct mld_depth_image_record {    /* 200 bytes, 8-byte aligned */
    int64_t counts[MLD_RESULT_TYPE_COUNT];  /* pixels of every DepthResultType */
    int64_t n_pixels;       /* grid_w * grid_h */
    int64_t n_depth;        /* pixels with depth >= 0 */
    int64_t n_cooperative;  /* pixels that left the lane-per-pixel route for k_depth_image_coop */
    int32_t flags;          /* MLD_DEPTH_IMAGE_FLAG_* */
    int32_t pad_;
} mld_depth_image_record;

typedef struct mld_depth_images mld_depth_images;
mld_depth_images* mld_depth_images_create(mld_ctx* ctx, int n_seq, const mld_params* params, const mld_camera* camera,
                                          const double T_cam_lidar[12], int* status_out);
void mld_depth_images_destroy(mld_depth_images* di);
const char* mld_depth_images_last_error(const mld_depth_images* di);
int mld_depth_images_render_device(mld_depth_images* di, const int32_t* const* map, const int32_t* const* index,
                                   const int64_t* index_len, const double* const* cam, const int64_t* n_points,
                                   const float* coeffs, const uint32_t* const* mask_dev, int x0, int y0, int step_x, int step_y,
                                   int grid_w, int grid_h, double* const* depth_out, float* const* depth32_out,
                                   uint8_t* const* type_out, mld_depth_image_record* record_out_dev);

/*
 * Region depths of a batch — the foreground depth of image RECTANGLES (a detector's 2-D box, a label blob's bounding box,
 * a tile of a matching prior), for n_seq independent sequences in one call.  A box is scanned like the window of
 * NeighborFinderPixel::getNeighbors (NeighborFinderPixel.cpp:70-79) with the box's own integer edges, of
 * ANY size, and its points go through the first-local-maximum histogram of PointHistogram::FilterPointsMinDistBlob
 * (HistogramPointDepth.cpp:30-100, row B3).  Besides the histogram's bin the record holds the count, the smallest, the
 * largest and the EXACT median depth and the nearest point.  Optionally the points of a ground plane are left out, so that
 * the road under a car does not answer for the car.  No frame slot, no synchronisation; the record holds only counts, order
 * statistics and bin borders, so the output does not depend on the order in which the GPU meets the points.
 *
 * Inputs: map[s], index[s], index_len[s], cam[s] and n_points[s] are the arrays mld_projected_clouds_export_device writes,
 * with the same meaning and the same bad-input rule as in the other objects that read them: a map value other than -1
 * outside [0, index_len[s]) and an index value outside [0, n_points[s]) make the cell EMPTY and set
 * MLD_REGION_FLAG_BAD_INPUT in the record of every box that contains the cell; no read leaves the arrays as the host tables
 * size them.  The depth of an occupied cell is the camera-frame z of its point, cam[s][3 * index[s][map value] + 2].  A z
 * that is not > 0 (zero, negative, NaN) is bad input too: the point is skipped and the flag is set.
 * mask_dev (optional table, optional entries): mask_dev[s] is the plane's inlier bitmask over the ORIGINAL point index, as
 * mld_semantic_planes_estimate_device and mld_ransac_planes_estimate_device write it (ceil(n_points[s] / 32) words).  A
 * point whose bit is set is excluded and counted in n_ground.  NULL: that sequence excludes nothing.
 * boxes[s]: n_boxes[s] x 4 int32 (x0, y0, x1, y1), both corners inclusive, 0 <= n_boxes[s] <= max_boxes (DEVICE memory; NULL
 * with n_boxes[s] == 0).  A box is clipped to [0, W - 1] x [0, H - 1]; the rows and columns scanned are those of
 * NeighborFinderPixel.cpp:70-79 for the same edges.  A box with x1 < x0 or y1 < y0, or one that the clipping leaves nothing
 * of, is EMPTY.
 * record_out[s]: n_boxes[s] records (DEVICE memory, 8-byte aligned; NULL with n_boxes[s] == 0), record b for box b, every one
 * written completely on every call and nothing else touched.
 *
 * The record.  "Counted points" are the occupied cells of the clipped box with z > 0 whose mask bit is not set.
 *   n_points      counted points
 *   n_ground      points with z > 0 that the mask excluded
 *   n_seg         counted points with hist_lower <= z < hist_higher; 0 without a bin
 *   flags         MLD_REGION_FLAG_BAD_INPUT 1, _EMPTY_BOX 2, _HIST_FOUND 4, _HIST_CAPPED 8, _HAS_MASK 16 (the sequence has a
 *                 mask, whatever the box holds)
 *   nearest_orig  the original index of the counted point with the smallest z; among equal z the first in row-major scan
 *                 order (rows from the top, columns from the left); -1 without a counted point
 *   clip          the clipped box (x0, y0, x1, y1); all -1 for an EMPTY box
 *   z_min, z_max, z_median   over the z of the counted points.  z_median is the element of rank (n_points - 1) / 2 (0-based,
 *                 integer division) in ascending order: an element of the set, never an interpolation.  All three are -1
 *                 with n_points == 0.
 *   hist_lower, hist_higher  the borders FilterPointsMinDistBlob returns for the z of the counted points with
 *                 histogram_segmentation_bin_witdh and histogram_segmentation_min_pointcount, every quirk kept: `int maxDist`
 *                 from ceil, binCount = (int)(maxDist / binWidth + 1), binCount <= 1 fails, the bin index of
 *                 Histogram::AddElement ((int)min(|min(z, 1e10) / binWidth|, binCount - 1)), the first bin that reaches the
 *                 minimal count and exceeds every earlier one, the scan ends at the first bin that decreases, and a bin of
 *                 zero points behind a bin with points fails the whole rule.  -1 / -1 when the rule returns false.  (The
 *                 depth path clamps z to 999 m before this rule, DepthEstimator.cpp:743; here z is taken as it is.  Where the
 *                 reference converts a double beyond the int range - a z or a bin count of 2^31 and more - the values
 *                 saturate at 2^31 - 1.)
 * Histogram storage: the histogram is kept relative to the bin of z_min, MLD_REGION_HIST_BINS bins long.  If the rule would
 * have to look at a bin beyond them - a run of bins that never decreases and never empties over more than
 * MLD_REGION_HIST_BINS * binWidth metres - the record gets MLD_REGION_FLAG_HIST_CAPPED and no bin (borders -1, n_seg 0, no
 * HIST_FOUND); nothing else of the record changes.
 *
 * mld_region_depths_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences of
 *   up to max_boxes (>= 1) boxes each.  Of params only histogram_segmentation_bin_witdh and
 *   histogram_segmentation_min_pointcount are read, of camera only width and height; both are copied.  All memory is
 *   allocated here, none per call:
 *     device  64 * n_seq bytes        (the descriptors)
 *     pinned  16 * 64 * n_seq bytes   (the descriptor ring)
 *   Judged in this order, the context LAST and nothing of it used before: n_seq and max_boxes; params and camera (null:
 *   MLD_ERR_INVALID_ARG); then
 *     MLD_ERR_INVALID_ARG   a bin width that is not finite or not > 0; an image size below 1 x 1
 *     MLD_ERR_CAPACITY      an image larger than 65535 pixels on a side or 2^30 pixels in all
 *     MLD_ERR_CAPACITY      n_seq * max_boxes beyond 2^31 - 1 (blocks of a launch)
 *     MLD_ERR_INVALID_ARG   a null context
 *   Returns NULL on failure with the reason in *status_out (optional) and the text in
 *   mld_region_depths_last_error(NULL).  Destroy the object before its context.
 *
 * mld_region_depths_collect_device: HOST tables of n_seq entries, consumed before the call returns; every array they name is
 * DEVICE memory.  Asynchronous on the context's stream: no synchronisation, no host read of device data, no runtime call per
 *   sequence, nothing allocated per call, no global atomics, no floating-point accumulation, two launches: the descriptor
 *   upload and k_region_depths, ONE BLOCK PER BOX (256 threads; a call's grid is n_seq times its largest n_boxes[s]; a call
 *   without a box launches nothing).  The block walks the rows of the clipped box with coalesced loads of the map, eight
 *   cells per thread in flight, gathers index, z and the mask bit, and reduces count, minimum, maximum and nearest point.
 *   A box of up to MLD_REGION_LIST_CAPACITY counted points keeps their z in LDS and takes the histogram, n_seg and the
 *   median from that list; a larger box scans its cells again for the histogram and for n_seg, and for the median until the
 *   values still in question fit the list.  The median is selected in both routes by the same radix passes of 8 bits over
 *   the bit pattern of z (positive doubles order as their bit patterns), from the highest bit in which z_min and z_max
 *   differ downwards, so the record is the same bit for bit on either route.  The work
 *   of a block follows the cells of its box: a box without a counted point leaves after the first scan, a box of one value
 *   needs no radix pass.  The device arrays must stay valid until the work has run.  Like a context, the object serves one
 *   call at a time.
 *   MLD_ERR_INVALID_ARG with a text naming the function and the argument (mld_region_depths_last_error; "null object (rd)"
 *   of NULL for a null object) on: a null object, a null table map, index, index_len, cam, n_points, boxes, n_boxes or
 *   record_out, a negative count, n_boxes[s] beyond max_boxes, a null map array (index, cam: where index_len[s],
 *   n_points[s] > 0; boxes, record_out: where n_boxes[s] > 0), an int32 array that is not 4-byte aligned, an f64 or record
 *   array that is not 8-byte aligned.  MLD_ERR_CAPACITY on n_points[s] or index_len[s] beyond 8 388 607.
 * In libmld_hip_ab.so only, MLD_REGION_LIST_CAPACITY=<n> in the environment (0 .. 2048), read at create, sets the capacity
 * of the list: 0 sends every box through the re-scanning route.
 */
#define MLD_REGION_LIST_CAPACITY 2048  /* z values of a box held in LDS (16 KiB) */
#define MLD_REGION_HIST_BINS 512       /* bins of the histogram held in LDS, from the bin of z_min on (2 KiB) */
enum {
    MLD_REGION_FLAG_BAD_INPUT = 1,
    MLD_REGION_FLAG_EMPTY_BOX = 2,
    MLD_REGION_FLAG_HIST_FOUND = 4,
    MLD_REGION_FLAG_HIST_CAPPED = 8,
    MLD_REGION_FLAG_HAS_MASK = 16
};

typedef struct mld_region_depth {    /* 80 bytes, 8-byte aligned */
    int32_t n_points;       /* counted points */
    int32_t n_ground;       /* points the mask excluded */
    int32_t n_seg;          /* counted points inside the histogram's bin */
    int32_t flags;          /* MLD_REGION_FLAG_* */
    int32_t nearest_orig;   /* original index of the nearest counted point, or -1 */
    int32_t clip[4];        /* the clipped box x0, y0, x1, y1; -1 when empty */
    int32_t pad_;
    double z_min, z_max, z_median;
    double hist_lower, hist_higher;
} mld_region_depth;

typedef struct mld_region_depths mld_region_depths;
mld_region_depths* mld_region_depths_create(mld_ctx* ctx, int n_seq, int64_t max_boxes, const mld_params* params,
                                            const mld_camera* camera, int* status_out);
void mld_region_depths_destroy(mld_region_depths* rd);
const char* mld_region_depths_last_error(const mld_region_depths* rd);
int mld_region_depths_collect_device(mld_region_depths* rd, const int32_t* const* map, const int32_t* const* index,
                                     const int64_t* index_len, const double* const* cam, const int64_t* n_points,
                                     const uint32_t* const* mask_dev, const int32_t* const* boxes, const int64_t* n_boxes,
                                     mld_region_depth* const* record_out);

/*
 * Nearest-return depths of a batch — the main path on the k closest returns of a feature instead of the returns of a fixed
 * rectangle, for n_seq independent sequences in one call.  A feature whose pixelarea_search window holds too few returns
 * (MLD_RadiusSearchInsufficientPoints) gets no depth from the depth path; the reference's answer is neighbor_search_mode 1
 * (parameters.yaml:5, NeighborFinderKdd: the nnSearch_count nearest returns, or all within radiusSearch_radius), which it
 * ships unfinished.  This object is that search over the pixel map, as ONE rule of integers with both of its modes as
 * corners: `count` nearest with a generous `radius`, or everything within `radius` with `count` at its maximum.  It runs on
 * the arrays mld_projected_clouds_export_device wrote (pixel map, _pointIndex, camera-frame cloud).
 *
 * The neighbour rule, for a feature (u, v), radius R and count k:
 *   centre cell   cx = (int)floor(clamp(u, -(R + 1), W + R)), cy = (int)floor(clamp(v, -(R + 1), H + R)), the clamp in f64
 *                 ahead of the cast: a feature far outside the image has an empty disc.  A non-finite u or v gives no
 *                 list, MLD_NEAREST_FLAG_NONFINITE_FEATURE and type 2.
 *   candidates    the cells (x, y) with 0 <= x < W, 0 <= y < H and d2 = (x - cx)^2 + (y - cy)^2 <= R * R whose map value m
 *                 is not -1, with 0 <= m < index_len and 0 <= index[m] < n_points.  A map value other than -1 that fails
 *                 those bounds makes the cell EMPTY and sets MLD_NEAREST_FLAG_BAD_INPUT on the features whose disc holds
 *                 it; no read leaves the arrays as the host tables size them.
 *   the list      the candidates in ascending (d2, y, x); the first min(n_in_radius, k) of them.
 * Two differences from the reference's finder, both deliberate: the pixel map holds ONE return per pixel (the first wins,
 * NeighborFinderPixel.cpp:38-55), so this is a search over cells, not over the sub-pixel positions of all returns; and it
 * is EXACT - the list is a function of the map alone - where FLANN's randomised kd-trees are approximate.
 * The list's points, in that order, then go through the main path as mld_feature_traces runs it: n_nb <
 * radiusSearch_count_min (compared as unsigned) gives type 2; the histogram segmentation with the 999 m clamp; the
 * max-spanning triangle, or the first three points; the planarity test, the viewing ray through the exact (u, v) - not
 * through the cell -, Hyperplane::Through, the orthogonality test, the thresholds, cut-behind-camera.  The road fallback
 * does not run here.
 *
 * mld_nearest_depth, one per feature; every record is written completely on every call:
 *   type          the main path's DepthResultType
 *   n_in_radius   candidates in the disc: always complete, also beyond k
 *   n_nb          entries of the list: min(n_in_radius, k)
 *   n_seg         points the segmentation kept (n_nb with the histogram off; 0 where it failed or was not reached)
 *   d2_first, d2_last   squared pixel distance of the first and of the last list entry; -1 without a list
 *   nearest_orig  original index of the first list entry, or -1
 *   flags         MLD_NEAREST_FLAG_BAD_INPUT 1, MLD_NEAREST_FLAG_NONFINITE_FEATURE 2
 *   depth         -1 unless type == MLD_Success
 *   nearest_z     camera z of the first list entry; NaN without one
 *   corner_vis    visible indices of the triangle's corners, -1 without corners
 *
 * mld_nearest_depths_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences
 *   of up to max_features (1 .. 16 777 216) features each, with radius in 1 .. MLD_NEAREST_MAX_RADIUS and count in
 *   1 .. MLD_NEAREST_MAX_COUNT.  params and camera are copied: pass the values the context was created with.  No
 *   transform is taken: nothing here reads it.  All memory is allocated here, none per call:
 *     device  72 * n_seq bytes        (the descriptors)
 *     pinned  16 * 72 * n_seq bytes   (the descriptor ring)
 *   The sizes are checked before the context is looked at (n_seq, max_features, then radius and count:
 *   MLD_ERR_INVALID_ARG with a text naming the argument), then the context, then params and camera (null), and then,
 *   still without a use of the context:
 *     MLD_ERR_UNSUPPORTED_MODE  do_use_PCA (the eigen-solve is a tolerance path, the records promise equality) and
 *                               set_all_depths_to_zero
 *     the refusals of mld_create for a parameter set and a camera, with its status codes and texts (neighbor_search_mode
 *     other than 0 among them: the parameter set stays the one the context runs with)
 *   Returns NULL on failure with the reason in *status_out (optional) and the text in
 *   mld_nearest_depths_last_error(NULL).  Destroy the object before its context.
 *
 * mld_nearest_depths_collect_device (uv[s] 2 x n_features[s] f64 column-major) and
 * mld_nearest_depths_collect_tracks_device (tracklet layer: u[s], v[s] f32; u = (double)truncf(u), likewise v, exactly as
 * mld_feature_traces_collect_tracks_device): HOST tables of n_seq entries, consumed before the call returns; every array
 * they name is DEVICE memory, naturally aligned for its element type (the records: 8 bytes).
 *   n_features[s], map[s], index[s], index_len[s], cam[s], n_points[s]   as mld_feature_traces_collect_device takes them
 *   record_out[s]       n_features[s] records
 *   nb_out              optional (the table, or single entries): list_capacity x n_features[s] int32, feature i's row at
 *                       i * list_capacity: the visible indices of the list in its order.  The first min(n_nb,
 *                       list_capacity) entries of a row are written and nothing behind them is touched.
 *   list_capacity       0 .. count; with 0 no list array is needed or written.
 *   Asynchronous on the context's stream: no synchronisation, no host read of device data, no runtime call per sequence,
 *   nothing allocated per call, no global atomics, no floating-point accumulation, two launches: the descriptor upload
 *   and k_nearest_depths, ONE WAVEFRONT PER FEATURE.  The wavefront reads the disc in square stages of half size 4, 8, 16,
 *   32, 64 (capped at radius) around the centre cell, only the new cells of each, and keeps a histogram of d2 in LDS; as
 *   soon as a stage has shown count candidates within its inscribed circle the SEARCH is over - the cut-off distance
 *   comes from the histogram, the candidates up to it are gathered from the small disc they lie in and ranked by
 *   (d2, y, x) - and the cells of the later stages are only counted, for n_in_radius and BAD_INPUT.  The device arrays must
 *   stay valid until the work has run.  Like a context, the object serves one call at a time.
 *   MLD_ERR_INVALID_ARG with a text naming the function and the argument (mld_nearest_depths_last_error; "null object
 *   (nd)" of NULL for a null object) on: a null object, a null table uv / u / v, n_features, map, index, index_len, cam,
 *   n_points or record_out, a null uv / u / v, map or record_out array of a sequence with features (index, cam: where
 *   index_len[s], n_points[s] > 0), a negative count, list_capacity outside 0 .. count, an int32 or float array that is
 *   not 4-byte aligned, an f64 array or record_out that is not 8-byte aligned.  MLD_ERR_CAPACITY on n_features[s] beyond
 *   max_features and on n_points[s] or index_len[s] beyond 8 388 607.
 */
#define MLD_NEAREST_MAX_RADIUS 64   /* pixels */
#define MLD_NEAREST_MAX_COUNT 256   /* entries of a list */
enum { MLD_NEAREST_FLAG_BAD_INPUT = 1, MLD_NEAREST_FLAG_NONFINITE_FEATURE = 2 };

typedef struct mld_nearest_depth {      /* 64 bytes, 8-byte aligned */
    int32_t type;           /* DepthResultType at the end of the main path */
    int32_t n_in_radius;    /* candidates in the disc */
    int32_t n_nb, n_seg;    /* entries of the list; those the segmentation kept */
    int32_t d2_first, d2_last;  /* squared pixel distances of the first and the last list entry, -1 without a list */
    int32_t nearest_orig;   /* original index of the first list entry, or -1 */
    int32_t flags;          /* MLD_NEAREST_FLAG_* */
    double  depth;          /* -1 unless type == MLD_Success */
    double  nearest_z;      /* camera z of the first list entry, NaN without one */
    int32_t corner_vis[3];  /* visible indices of the corners, -1 without corners */
    int32_t pad_;
} mld_nearest_depth;

typedef struct mld_nearest_depths mld_nearest_depths;
mld_nearest_depths* mld_nearest_depths_create(mld_ctx* ctx, int n_seq, int64_t max_features, int radius, int count,
                                              const mld_params* params, const mld_camera* camera, int* status_out);
void mld_nearest_depths_destroy(mld_nearest_depths* nd);
const char* mld_nearest_depths_last_error(const mld_nearest_depths* nd);
int mld_nearest_depths_collect_device(mld_nearest_depths* nd, const double* const* uv, const int64_t* n_features,
                                      const int32_t* const* map, const int32_t* const* index, const int64_t* index_len,
                                      const double* const* cam, const int64_t* n_points, int list_capacity,
                                      mld_nearest_depth* const* record_out, int32_t* const* nb_out);
int mld_nearest_depths_collect_tracks_device(mld_nearest_depths* nd, const float* const* u, const float* const* v,
                                             const int64_t* n_features, const int32_t* const* map, const int32_t* const* index,
                                             const int64_t* index_len, const double* const* cam, const int64_t* n_points,
                                             int list_capacity, mld_nearest_depth* const* record_out, int32_t* const* nb_out);

/*
 * Row-growth depths of a batch — the reference's second depth segmentation (do_use_depth_segmentation: 1, the value the
 * shipped parameters.yaml:74 holds) for n_seq independent sequences: HelperLidarRowSegmentation cuts the visible list into
 * lidar rows, grows a region along the row of the feature's nearest return and along one neighbouring row, and
 * DepthEstimator::CalculateDepth (DepthEstimator.cpp:512-558) runs the triangle path on the grown points and answers
 * MLD_SuccessRegionGrowing.  The reference keeps the mode behind a throw (:608) and mld_create keeps refusing it; this
 * object is the mode as its code states it, quirks included, on the arrays mld_projected_clouds_export_device wrote.  It
 * segments by 3-D continuity along the scan where the main path segments by a depth histogram.  All arithmetic is f64
 * without contraction; every result is an integer or a float bit pattern.
 *
 * The rule.  Rows (HelperLidarRowSegmentation.cpp:18-46): walking the visible list in order with lastX = (double)INT_MIN,
 *   visible point i opens a row iff x_i > lastX + 50 (strictly), then lastX = x_i; point 0 always opens row 0.  Rows are
 *   contiguous ranges of the visible list: row r is [row_start[r], row_start[r + 1]).  The segmenter assumes that u falls
 *   along a beam and jumps up at the next one, and checks nothing; a cloud scanned the other way is a few very long rows.
 * The seed (DepthEstimator.cpp:509-530, :687-724): the neighbours of the narrow window in scan order (n_nb; (unsigned)n_nb <
 *   radiusSearch_count_min: type 2).  CalculateNearestPoint folds with a FLOAT accumulator: m = +inf; z_i < (double)m: m =
 *   (float)z_i, the seed is i - two returns closer than float resolution resolve either way.  No seed (every z NaN or
 *   +inf): MLD_HistogramNoLocalMax at once.  z_seed > (double)treshold_depth_max: MLD_TresholdDepthGlobalGreaterMax at
 *   once, whether or not treshold_depth_enabled is set.
 * The second seed (HelperLidarRowSegmentation.cpp:68-157, :277-300), on the rows r - 1 and r + 1 of the seed's row r where
 *   they exist: the first column c with x_c < fx && x_{c-1} >= fx (x_{-1} = INT_MIN: column 0 does not match); none: the
 *   row has no point.  Else c if |p_c - f|^2 < |p_c - p_{c-1}|^2 - the second distance is between the two returns - else
 *   c - 1.  Neither row: state -1.  Both: the top row first iff distTop < distBottom (2-D, to the feature; a tie puts the
 *   bottom row first).  The first of them whose 3-D distance to the seed is <= maxDistSeedToSeed, else state -2.
 * getMaxDist(thr, start, grad, z_seed) (:302-313): start where z_seed <= thr, else start + (z_seed - start) * grad - the
 *   delta is taken from start, not from thr.
 * Growth (:159-275, :359-368): the call sites hand (maxDistNeighborToSeed, maxDistNeighbor) to the parameters named
 *   (maxDistanceNeighbor, maxDistanceSeed) - the roles are swapped.  Distances are sqrt((dx * dx + dy * dy) + dz * dz).  The
 *   seed's row is grown with count / 2 (int division; -1 stays -1), then the second seed's row with count, onto the same
 *   list; the seeds themselves are never in it.  count < 0: up the columns until the row ends, d(p, seed) >
 *   maxDistanceSeed or d(p, last) > maxDistanceNeighbor, then down the columns by the same rule WITHOUT resetting `last`.
 *   count >= 0: a two-pointer merge takes the side whose next point is closer to the seed ('<=' takes the upper side), no
 *   neighbour test; it ends as soon as EITHER side runs out, the taken point is farther than maxDistanceSeed, or the list
 *   holds count entries.  Nothing added by the second call: state -3, else state 1.
 * The depth (DepthEstimator.cpp:551-556, :903-1036), state 1: CalculateDepthSegmented on the grown list in its order - the
 *   max-spanning triangle or the first three points, the planarity check if configured, the viewing ray through the exact
 *   (u, v), the thresholds on the list's min and max z; no count test, no histogram.  MLD_Success becomes
 *   MLD_SuccessRegionGrowing.  Everything else - the states -1, -2, -3 and a failed triangle - decides nothing: the
 *   ordinary path runs and its result stands (:564-572).  The whole mode is therefore: this stage's result where it decides
 *   (type 20, the early 4, the early 3), the product's result everywhere else - which the in-place merge below writes.
 *
 * mld_row_growth_params: the eight depth_segmentation_* values with the reference's names and spelling;
 *   mld_row_growth_params_default gives DepthEstimatorParameters.h:52-60, mld_row_growth_params_yaml the shipped
 *   parameters.yaml:77-91.  depth_segmentation_max_pointcount is stored as a double there and truncated at the call.
 *
 * mld_row_growth_cloud, one per sequence, 16 bytes in DEVICE memory, written completely by every segment call:
 *   n_rows        rows of the visible list: complete, also beyond row_capacity
 *   n_vis         visible points segmented: min(n_visible, capacity[s])
 *   longest_row   points of the longest row
 *   flags         MLD_ROW_GROWTH_FLAG_ROWS_TRUNCATED: n_rows > row_capacity
 * mld_row_growth, one per feature, 72 bytes; every record is written completely on every call:
 *   type          MLD_SuccessRegionGrowing, the early MLD_TresholdDepthGlobalGreaterMax, the early MLD_HistogramNoLocalMax,
 *                 MLD_RadiusSearchInsufficientPoints, or MLD_Unspecified: this stage decides nothing
 *   state         calculateNeighborPoints' result 1, -1, -2, -3; 0 when not reached
 *   grown_type    what CalculateDepthSegmented gave on the grown list; 0 when not reached
 *   flags         MLD_ROW_GROWTH_FLAG_*
 *   n_nb          neighbours in the narrow window
 *   seed_vis, second_vis   visible indices of the two seeds, -1 without
 *   seed_row, second_row   their rows, -1 without
 *   n_first       list entries that came from the seed's row
 *   n_grown       list entries in all: complete, also beyond MLD_ROW_GROWTH_MAX_LIST
 *   corner_vis    visible indices of the triangle's corners, -1 without corners
 *   depth         -1 unless type == MLD_SuccessRegionGrowing
 *   seed_z        camera z of the seed, NaN without one
 * Flags: BAD_INPUT - a map, index or row value points outside its array (map values as at mld_nearest_depths; a row whose
 *   bounds leave [0, min(n_vis, index_len)] or run backwards is empty; a row point whose index lies outside the cloud ends
 *   a loop as the row's end would; a seed that no row holds ends the feature with MLD_Unspecified, state 0); no read leaves
 *   the arrays as the host tables size them.  NONFINITE_FEATURE - type 2.  ROWS_TRUNCATED - every feature of that sequence
 *   gets MLD_Unspecified, state 0 and nothing else is looked at.  LIST_CAPPED - unbounded growth passed
 *   MLD_ROW_GROWTH_MAX_LIST entries: n_grown is complete, the type is MLD_Unspecified, the tail is not run.
 *
 * mld_row_growth_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences of up
 *   to max_features (1 .. 16 777 216) features and max_points (1 .. 8 388 607) visible points each, with row tables of
 *   row_capacity (1 .. MLD_ROW_GROWTH_MAX_ROWS) rows.  params, growth and camera are copied; params->do_use_depth_segmentation
 *   may hold either value.  All memory is allocated here, none per call:
 *     device  n_seq * (8 * ceil(max_points / 64) + 16 * ceil(max_points / 1024) + 4 + 152) bytes   (break mask per 64 points,
 *             break count and gaps per 1024 points; the descriptors of both calls)
 *     pinned  16 * 152 * n_seq bytes   (the two descriptor rings)
 *   The sizes are checked before the context is looked at (n_seq, max_features, max_points, row_capacity:
 *   MLD_ERR_INVALID_ARG with a text naming the argument), then the context, then params, growth, camera and T_cam_lidar
 *   (null), the count (-1, or 0 .. MLD_ROW_GROWTH_MAX_COUNT), and then, still without a use of the context, what
 *   mld_nearest_depths_create refuses of a parameter set and a camera, with its codes and texts (do_use_PCA and
 *   set_all_depths_to_zero first), a transform that is not finite, and a wide window of more than 1024 cells.  Returns NULL
 *   on failure with the reason in *status_out (optional) and the text in mld_row_growth_last_error(NULL).  Destroy the
 *   object before its context.
 *
 * mld_row_growth_segment_device, the cloud stage, once per cloud: HOST tables of n_seq entries, consumed before the call
 *   returns; every array they name is DEVICE memory.
 *   uv[s], capacity[s], n_visible_dev   as mld_projected_clouds_export_device wrote them: 2 x capacity[s] f64 and the int64
 *                       array of n_seq counts.  capacity[s] <= max_points; uv[s] may be NULL where capacity[s] is 0.
 *   row_start_out[s]    row_capacity + 1 int32.  Entries 0 .. min(n_rows, row_capacity) are written - row_start[n_rows] is
 *                       n_vis where nothing was truncated - and nothing behind them is touched.
 *   cloud_out_dev       n_seq records.
 *   Asynchronous on the context's stream, three kernels behind the descriptor upload (k_rg_pass, k_rg_scan, k_rg_write: the
 *   pass / scan / write compaction over the break flags), no atomics, no synchronisation, nothing comes back to the host.
 *
 * mld_row_growth_collect_device (uv[s] 2 x n_features[s] f64) and mld_row_growth_collect_tracks_device (u[s], v[s] f32,
 *   truncated as at mld_nearest_depths_collect_tracks_device), the feature stage: HOST tables as at
 *   mld_nearest_depths_collect_device, plus
 *   vis_uv[s]           the uv array the segment call read, at least 2 x index_len[s] f64
 *   row_start[s], cloud_dev   what the segment call wrote for these clouds; n_rows is read on the GPU
 *   list_capacity       0 .. MLD_ROW_GROWTH_MAX_LIST
 *   record_out[s]       n_features[s] records
 *   grown_out           optional (the table, or single entries): list_capacity x n_features[s] int32, feature i's row at
 *                       i * list_capacity: the visible indices of the grown list in its order.  The first min(n_grown,
 *                       list_capacity, MLD_ROW_GROWTH_MAX_LIST) entries of a row are written, nothing behind them is touched.
 *   depth_io, type_io   optional (the tables, or single entries): n_features[s] f64 (tracks form: f32) and int32, the
 *                       outputs of mld_calculate_depths_device (the tracklet layer's) for these features.  Where the
 *                       record decides (type 20, 4 or 3) depth and type are overwritten; everywhere else they are not
 *                       touched.  With them the batch holds what CalculateDepth returns under do_use_depth_segmentation: 1.
 *   Asynchronous on the context's stream, two launches: the descriptor upload and k_row_growth, ONE WAVEFRONT PER FEATURE.
 *   MLD_ERR_INVALID_ARG with a text naming the function and the argument (mld_row_growth_last_error; "null object (rg)" of
 *   NULL for a null object) on what mld_nearest_depths_collect_device refuses and on a null table vis_uv or row_start, a
 *   null cloud_dev, a null vis_uv (index_len[s] > 0) or row_start array of a sequence with features, list_capacity out of
 *   range, an array that is not naturally aligned.  MLD_ERR_CAPACITY as there.
 */
#define MLD_ROW_GROWTH_MAX_COUNT 256    /* depth_segmentation_max_pointcount */
#define MLD_ROW_GROWTH_MAX_LIST 1024    /* entries of a grown list that are kept */
#define MLD_ROW_GROWTH_MAX_ROWS 65536   /* row_capacity */
enum { MLD_ROW_GROWTH_FLAG_BAD_INPUT = 1, MLD_ROW_GROWTH_FLAG_NONFINITE_FEATURE = 2, MLD_ROW_GROWTH_FLAG_ROWS_TRUNCATED = 4,
       MLD_ROW_GROWTH_FLAG_LIST_CAPPED = 8 };

typedef struct mld_row_growth_params {  /* 64 bytes */
    double depth_segmentation_max_treshold_gradient;                        /* DepthEstimatorParameters.h:52 */
    double depth_segmentation_max_neighbor_distance;                        /* :53 */
    double depth_segmentation_max_neighbor_distance_gradient;               /* :54 */
    double depth_segmentation_max_neighbor_to_seedpoint_distance;           /* :55 */
    double depth_segmentation_max_seedpoint_to_seedpoint_distance_gradient; /* :56 */
    double depth_segmentation_max_seedpoint_to_seedpoint_distance;          /* :57 */
    double depth_segmentation_max_neighbor_to_seedpoint_distance_gradient;  /* :58 */
    int32_t depth_segmentation_max_pointcount;                              /* :60  -1: unbounded */
    int32_t pad_;
} mld_row_growth_params;

typedef struct mld_row_growth_cloud {   /* 16 bytes */
    int32_t n_rows, n_vis, longest_row, flags;
} mld_row_growth_cloud;

typedef struct mld_row_growth {         /* 72 bytes, 8-byte aligned */
    int32_t type;           /* 20, the early 4, the early 3, 2, or MLD_Unspecified */
    int32_t state;          /* 1, -1, -2, -3; 0 when not reached */
    int32_t grown_type;     /* CalculateDepthSegmented on the grown list; 0 when not reached */
    int32_t flags;          /* MLD_ROW_GROWTH_FLAG_* */
    int32_t n_nb;           /* neighbours in the narrow window */
    int32_t seed_vis, second_vis;  /* visible indices of the seeds, -1 without */
    int32_t seed_row, second_row;  /* their rows, -1 without */
    int32_t n_first, n_grown;      /* list entries from the seed's row; in all */
    int32_t corner_vis[3];  /* visible indices of the corners, -1 without corners */
    double  depth;          /* -1 unless type == MLD_SuccessRegionGrowing */
    double  seed_z;         /* camera z of the seed, NaN without one */
} mld_row_growth;

void mld_row_growth_params_default(mld_row_growth_params* g);
void mld_row_growth_params_yaml(mld_row_growth_params* g);

typedef struct mld_row_growth_unit mld_row_growth_unit;
mld_row_growth_unit* mld_row_growth_create(mld_ctx* ctx, int n_seq, int64_t max_features, int64_t max_points, int row_capacity,
                                           const mld_params* params, const mld_row_growth_params* growth,
                                           const mld_camera* camera, const double T_cam_lidar[12], int* status_out);
void mld_row_growth_destroy(mld_row_growth_unit* rg);
const char* mld_row_growth_last_error(const mld_row_growth_unit* rg);
int mld_row_growth_segment_device(mld_row_growth_unit* rg, const double* const* uv, const int64_t* capacity,
                                  const int64_t* n_visible_dev, int32_t* const* row_start_out,
                                  mld_row_growth_cloud* cloud_out_dev);
int mld_row_growth_collect_device(mld_row_growth_unit* rg, const double* const* uv, const int64_t* n_features,
                                  const int32_t* const* map, const int32_t* const* index, const int64_t* index_len,
                                  const double* const* cam, const int64_t* n_points, const double* const* vis_uv,
                                  const int32_t* const* row_start, const mld_row_growth_cloud* cloud_dev, int list_capacity,
                                  mld_row_growth* const* record_out, int32_t* const* grown_out, double* const* depth_io,
                                  int32_t* const* type_io);
int mld_row_growth_collect_tracks_device(mld_row_growth_unit* rg, const float* const* u, const float* const* v,
                                         const int64_t* n_features, const int32_t* const* map, const int32_t* const* index,
                                         const int64_t* index_len, const double* const* cam, const int64_t* n_points,
                                         const double* const* vis_uv, const int32_t* const* row_start,
                                         const mld_row_growth_cloud* cloud_dev, int list_capacity,
                                         mld_row_growth* const* record_out, int32_t* const* grown_out, float* const* depth_io,
                                         int32_t* const* type_io);

/*
 * Merged sweeps of a batch — the last few lidar sweeps of n_seq independent sequences carried into the current lidar
 * frame and concatenated, current sweep first, in one call.  Most features get no depth because too few returns lie
 * around them (MLD_RadiusSearchInsufficientPoints); the usual remedy changes the cloud, not the search: the sweeps the
 * sensor delivered just before, moved by the ego-motion the SLAM loop already has, projected together with the current
 * one.  The pixel map keeps the FIRST return that lands in a cell (NeighborFinderPixel.cpp:38-55): with the current
 * sweep in front its returns keep their cells and the older sweeps only fill empty ones, so the order of the output
 * is part of the contract.  The merged cloud is a cloud as mld_set_clouds*_device takes it (16-byte records).
 *
 * The rule, for sequence s and sweep j (0: the current one) of n_sweeps, entry e = s * n_sweeps + j of the tables:
 *   record      n[e] records of stride_bytes at pts_dev[e]: x, y, z at offsets 0, 4, 8; the intensity where
 *               mld_pack_points_host takes it (offset 12 of a 16-byte record, 16 of a 32-byte one), as raw bits.
 *   transform   T[e]: 12 doubles in HOST memory, a row-major 3x4 matrix from sweep j's lidar frame to the current one,
 *               read before the call returns.  A NULL entry (a NULL table: every entry) is the identity: x, y, z are
 *               taken bit for bit, the sign of a zero included.  Otherwise, with x, y, z promoted to double,
 *                 x' = (float)(T[3] + (T[0] * x + (T[1] * y + T[2] * z)))      y', z' likewise from rows 1, 2
 *               in exactly this operation order, without contraction.
 *   dropped     NON-FINITE: one of x', y', z' is not finite.  OUT OF RANGE: r2 = x' * x' + (y' * y' + z' * z') in f32
 *               fails lo2 <= r2 && r2 <= hi2, with lo2 = min_range * min_range and hi2 = max_range * max_range made
 *               on the host in f32.  A record that is both counts as non-finite only.  min_range 0 with max_range
 *               +inf gates nothing.
 *   output      the kept records of sweep 0 in their order, then those of sweep 1, and so on, as packed 16-byte records
 *               {x', y', z', intensity bits} in merged_out[s]; the first min(n_kept, capacity[s]) of them are written
 *               and nothing behind them is touched.  The counts stay complete beyond the capacity.
 *
 * mld_sweep_merge_record, one per sequence, in DEVICE memory; every record is written completely on every call:
 *   n_in            records of all sweeps
 *   n_kept          n_in - n_nonfinite - n_out_of_range
 *   n_written       min(n_kept, capacity[s])
 *   n_nonfinite, n_out_of_range   the two reasons, each record under one
 *   kept[j]         kept records of sweep j, complete also beyond the capacity; 0 at and beyond n_sweeps
 *   flags           MLD_SWEEP_FLAG_TRUNCATED: n_kept > capacity[s]
 *
 * mld_sweep_merge_create: an object bound to `ctx` (its stream, its device) for calls of n_seq (1 .. 65536) sequences of
 *   up to max_sweeps (1 .. MLD_SWEEP_MAX_SWEEPS) sweeps of up to max_points (1 .. 8 388 607) points each, with
 *   max_sweeps * max_points <= 8 388 607: the merged cloud must fit the 23-bit point index of the pixel map.  All memory
 *   is allocated here, none per call; with I = max_sweeps * max_points:
 *     device  152 * max_sweeps * n_seq bytes        (the descriptors, one per sweep)
 *             n_seq * (8 * ceil(I / 64) + 8 * (ceil(I / 1024) + 1) + 72) bytes   (kept mask per 64 items, two counts per
 *                                                   1024 items, the totals)
 *     pinned  16 * 152 * max_sweeps * n_seq bytes   (the descriptor ring)
 *   The sizes are checked before the context is looked at, in the order n_seq, max_sweeps, max_points, their product
 *   (MLD_ERR_INVALID_ARG with a text naming the argument), then the context.  Returns NULL on failure with the reason
 *   in *status_out (optional) and the text in mld_sweep_merge_last_error(NULL).  Destroy the object before its context.
 *
 * mld_sweep_merge_run_device: HOST tables, consumed before the call returns; every array they name is DEVICE memory.
 *   pts_dev, n, T   n_seq * n_sweeps entries (T: optional, as above); the records 4-byte aligned
 *   capacity[s]     records merged_out[s] has room for
 *   merged_out[s]   16 * capacity[s] bytes, 4-byte aligned; may be NULL where capacity[s] or the sequence's n_in is 0
 *   sweep_out       optional (the table, or single entries): uint8 per written record, the sweep j it came from
 *   orig_out        optional likewise: int32 per written record, its index within its sweep; 4-byte aligned
 *   record_out_dev  n_seq records, 8-byte aligned
 *   Asynchronous on the context's stream: no synchronisation, no host read of device data, no runtime call per
 *   sequence, nothing allocated per call, no atomics, four launches: the descriptor upload, k_sm_pass (one load of 16
 *   bytes per record, the transform, the tests; a 64-bit mask per 64 items and two drop counts per 1024), k_sm_scan (per
 *   sequence: the prefixes, the kept records of every sweep) and k_sm_write (rank by popcount; only kept records below
 *   the capacity are loaded and transformed again and stored whole; one more block per sequence writes the record).
 *   The device arrays must stay valid until the work has run.  Like a context, the object serves one call at a time.
 *   The arguments are judged in this order, before anything is queued: the object; n_sweeps; the tables pts_dev and n;
 *   stride_bytes; min_range, max_range (each >= 0 and not NaN, min_range <= max_range); the tables capacity and
 *   merged_out; record_out_dev and its alignment; then per sequence its sweeps in order (n, pts_dev), its capacity and
 *   its output arrays.  MLD_ERR_INVALID_ARG with a text naming the function and the argument
 *   (mld_sweep_merge_last_error; "null object (sm)" of NULL for a null object) on: a null object, n_sweeps outside
 *   1 .. max_sweeps, a null table pts_dev, n, capacity or merged_out, a null record_out_dev, a stride other than 16 or
 *   32, a bad range, a negative n or capacity, a null pts_dev of a sweep with points, a null merged_out of a sequence
 *   with points and capacity, an array that is not aligned as said.  MLD_ERR_CAPACITY on n beyond max_points.
 */
#define MLD_SWEEP_MAX_SWEEPS 16
enum { MLD_SWEEP_FLAG_TRUNCATED = 1 };

typedef struct mld_sweep_merge_record {  /* 112 bytes, 8-byte aligned */
    int64_t n_in, n_kept, n_written, n_nonfinite, n_out_of_range;
    int32_t kept[MLD_SWEEP_MAX_SWEEPS];  /* per sweep, complete */
    int32_t flags;                       /* MLD_SWEEP_FLAG_* */
    int32_t pad_;
} mld_sweep_merge_record;

typedef struct mld_sweep_merge mld_sweep_merge;
mld_sweep_merge* mld_sweep_merge_create(mld_ctx* ctx, int n_seq, int max_sweeps, int64_t max_points, int* status_out);
void mld_sweep_merge_destroy(mld_sweep_merge* sm);
const char* mld_sweep_merge_last_error(const mld_sweep_merge* sm);
int mld_sweep_merge_run_device(mld_sweep_merge* sm, int n_sweeps, const void* const* pts_dev, const int64_t* n,
                               int stride_bytes, const double* const* T, float min_range, float max_range,
                               const int64_t* capacity, void* const* merged_out, uint8_t* const* sweep_out,
                               int32_t* const* orig_out, mld_sweep_merge_record* record_out_dev);

/*
 * Debug / parity getters (host buffers; each synchronises).
 *   mld_get_visible_count           -> _points_cs_image_visible.cols()         (DepthEstimator.cpp:192)
 *   mld_get_visible_image_points    -> getPointsCloudImageCs, 2 x Nvis col-major (:392-394)
 *   mld_get_point_index             -> PointcloudData::_pointIndex, Nvis int32   (:203)
 *   mld_get_cloud_camera_cs         -> getCloudCameraCs, 3 x N col-major float64 (:314-334)
 *   mld_get_pixel_map               -> NeighborFinderPixel::_img_points_lidar, W*H int32, index x + y*W,
 *                                      value = VISIBLE index or -1               (NeighborFinderPixel.cpp:38-55)
 *   mld_get_point_depth_cam_visible -> getPointDepthCamVisible(index)            (DepthEstimator.h:111-113)
 */
int mld_get_visible_count(mld_ctx* ctx, int slot, int64_t* n_visible);
/*
 * Which kernel answered the features of the slot's last BATCHED CalculateDepth call (mld_calculate_depths_device and the
 * tracklet entry points; no reference counterpart): `lane_path` = features the classification queued for the
 * lane-per-feature kernel, `handed_over` = features the wave-cooperative kernel worked on (lists beyond the capacities /
 * the budget of mld_set_list_capacity / mld_set_list_budget, windows wider than 32 cells, road fits whose error estimate
 * asks for the QR route; a feature handed over by the lane kernel counts in both).  The feedback for choosing capacities:
 * a wave-kernel feature costs ~10x a lane-path one.  Synchronises the context's stream.
 */
int mld_get_path_counts(mld_ctx* ctx, int slot, int64_t* lane_path, int64_t* handed_over);
int mld_get_visible_image_points(mld_ctx* ctx, int slot, double* uv_out, int64_t capacity);
int mld_get_point_index(mld_ctx* ctx, int slot, int32_t* index_out, int64_t capacity);
int mld_get_cloud_camera_cs(mld_ctx* ctx, int slot, double* xyz_out, int64_t capacity);
int mld_get_pixel_map(mld_ctx* ctx, int slot, int32_t* map_out, int64_t capacity);
int mld_get_point_depth_cam_visible(mld_ctx* ctx, int slot, int64_t visible_index, double* depth_out);

/*
 * Debug mode (ActivateDebugMode, DepthEstimator.h:85-87) — the debug vectors behind getCloudTriangleCorners /
 * getCloudRansacPlane (DepthEstimator.cpp:347-349, 396-398).
 *   mld_calculate_depth_debug  -> CalculateDepth plus `_points_triangle_corners` as filled by
 *                                 CalculatePlaneCorners (PlaneEstimationCalcMaxSpanningTriangle.cpp:20-35,
 *                                 called from DepthEstimator.cpp:916): corners_out is 9 x F column-major
 *                                 (corner1 xyz, corner2 xyz, corner3 xyz; camera frame) for every feature whose
 *                                 spanning triangle was found, NaN otherwise.  Feature order instead of the
 *                                 reference's unordered OpenMP push order.  Same depths/types as
 *                                 mld_calculate_depth; slower (every feature takes the wave-cooperative kernel).
 *   mld_get_ground_plane_cloud -> `_points_groundplane` (DepthEstimator.cpp:294-308): camera-frame coordinates of
 *                                 the slot's ground-plane inliers, ascending original index, filtered by
 *                                 ransac_plane_use_camx_treshold / ransac_plane_treshold_camx.  3 x n
 *                                 column-major; xyz_out == NULL only counts.
 */
int mld_calculate_depth_debug(mld_ctx* ctx, int slot, const double* uv_host, int64_t F, double* depth_out_host,
                              int32_t* type_out_host, double* corners_out_host);
int mld_get_ground_plane_cloud(mld_ctx* ctx, int slot, double* xyz_out, int64_t capacity, int64_t* n_out);

/* DepthCalculationStatistics counterpart: histogram of a resultType array (counts[MLD_RESULT_TYPE_COUNT]). */
int mld_result_histogram(const int32_t* types, int64_t F, int64_t counts[MLD_RESULT_TYPE_COUNT]);

/*
 * Measurement hooks for bench.py (HIP events on the context's stream).
 *   mld_kernel_time_ms: average duration in ms of the `which` kernel (0 = k_project_scatter, 1 = k_feature_fused,
 *   3 = k_feature_wave, 5 = k_classify) over the launches since mld_timing_reset, measured with hipEvents recorded
 *   around each launch when timing is enabled.
 */
int mld_timing_enable(mld_ctx* ctx, int enable);
int mld_timing_reset(mld_ctx* ctx);
int mld_kernel_time_ms(mld_ctx* ctx, int which, double* avg_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* MLD_H_ */
