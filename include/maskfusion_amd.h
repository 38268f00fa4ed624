/*
 * maskfusion_amd.h -- C ABI of the MI355X-native MaskFusion hot path (libmaskfusion_amd.so).
 *
 * Drop-in boundary for `MaskFusion::processFrame` and the `Model` operations it drives
 * (reference: martinruenz/maskfusion, Core/MaskFusion.h:45-307, Core/Model/Model.h:108-268).
 * The reference exposes a C++14 class over Eigen/OpenCV/OpenGL types; this ABI carries the same
 * operations over plain pointers and sizes.  include/maskfusion/MaskFusion.h is the header-only C++
 * facade with the reference's class/method names on top of it; INTEGRATION.md shows the binding a
 * MaskFusion maintainer adds.
 *
 * Conventions
 *   - 4x4 poses: 16 floats, COLUMN-major (memcpy-compatible with Eigen::Matrix4f::data()).
 *   - rgb: H*W*3 uint8 (FrameData::rgb, CV_8UC3); depth: H*W float32 metres, 0 = invalid
 *     (FrameData::depth, CV_32FC1); mask: H*W uint8 model ids (FrameData::mask, CV_8UC1) or NULL.
 *   - surfel record (Model::SurfelMap, Core/Model/Model.h:193-206): 12 floats
 *     {x,y,z,conf | colour(24-bit int as float),unused,initTime,lastTime | nx,ny,nz,radius}.
 *   - every function returns 0 on success or a negative MF_E* code; mf_last_error() has the text.
 *     No exceptions cross the ABI; a context is thread-compatible (one caller at a time), owns one HIP
 *     stream on one GPU, and holds no process-global state (unlike the reference's Resolution /
 *     Intrinsics / GPUSetup singletons, Core/Utils/Resolution.h:24-71, Core/Model/Model.h:54-89).
 *   - "_dev" entry points take DEVICE pointers (HBM-resident inputs); the others take host pointers.
 *   - The library needs a gfx950 GPU: mf_create() fails with MF_ENODEV otherwise.  There is no CPU path.
 */
#ifndef MASKFUSION_AMD_H_
#define MASKFUSION_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MF_OK 0
#define MF_EINVAL (-1)  /* bad argument */
#define MF_ENODEV (-2)  /* no usable GPU / HIP failure at init */
#define MF_EHIP (-3)    /* HIP runtime error (text in mf_last_error) */
#define MF_ENOMEM (-4)
#define MF_ESTATE (-5)  /* call not valid in this state */

typedef struct mf_ctx mf_ctx;

/* Constructor arguments of MaskFusion (Core/MaskFusion.h:47-53) that are live on the hot path, plus what the
 * reference reads from the Resolution / Intrinsics singletons (GUI/MainController.cpp:117-128) and the
 * compile-time surfel budgets (Core/CMakeLists.txt:27-28; Core/Model/Model.cpp:101-108). */
typedef struct mf_config {
    int32_t width, height;
    float fx, fy, cx, cy;
    int32_t device;               /* HIP device ordinal (MASKFUSION_GPU_SLAM) */
    int32_t time_delta;           /* timeDelta = 200 */
    float conf_global;            /* initConfidenceGlobal = 4 */
    float conf_object;            /* initConfidenceObject = 2 */
    float depth_cutoff;           /* depthCut = 3 */
    float icp_weight;             /* icpThresh = 10; >= 100 => geometric term only */
    int32_t fast_odom;            /* fastOdom = 0 */
    int32_t so3;                  /* so3 = 1 */
    int32_t pyramid;              /* pyramid = 1 (MaskFusion.cpp:60) */
    float max_depth_processed;    /* 20 (MaskFusion.cpp:57) */
    float outlier_coefficient;    /* Model::GPUSetup::outlierCoefficient = 0.9 (Model.h:85) */
    int32_t num_gsurfels;         /* MASKFUSION_NUM_GSURFELS = 9437184 */
    int32_t num_osurfels;         /* MASKFUSION_NUM_OSURFELS = 1048576 */
    int32_t enable_multiple_models; /* setEnableMultipleModels; 0 == "-static" */
    int32_t model_spawn_offset;   /* modelSpawnOffset = 20 (Core/MaskFusion.h:51) */
    int32_t track_all_models;     /* MaskFusion::trackAllModels = true (Core/MaskFusion.h:396) */
    int32_t max_models;           /* upper bound on live models (the reference: 256 ids) */
    int32_t rgb_only;             /* rgbOnly = 0 (Core/MaskFusion.h:169): photometric term only */
    int32_t pose_log_capacity;    /* enablePoseLogging (Core/MaskFusion.h:402): entries kept per model; 0 = off */
    int32_t reserved[3];
} mf_config;

/* Fills *cfg with the reference's constructor defaults for a WxH camera. */
int mf_default_config(mf_config* cfg, int32_t width, int32_t height, float fx, float fy, float cx, float cy);

/* MaskFusion::MaskFusion (Core/MaskFusion.cpp:24-120) */
int mf_create(const mf_config* cfg, mf_ctx** out);
/* MaskFusion::~MaskFusion (Core/MaskFusion.cpp:122-142) */
void mf_destroy(mf_ctx* ctx);
const char* mf_last_error(const mf_ctx* ctx);

/* MaskFusion::processFrame (Core/MaskFusion.h:69-70, Core/MaskFusion.cpp:200-607).
 * mask/class_ids may be NULL (n_masks = 0); in_pose16 may be NULL.  The caller's buffers are copied into pinned staging memory before
 * the call returns (they may be reused at once); the upload and the frame itself are ENQUEUED -- the call does not wait for THIS frame
 * (it keeps the host at most two frames ahead: it waits for frame k-2 before enqueueing frame k's upload; a multi-model frame also
 * waits once for the label stage's decision).  Every getter below synchronises first, so
 * processFrame(...); getCurrPose() reads this frame's pose as upstream; mf_sync() waits explicitly.
 * mf_set_param("hostInputAsync", 0) restores the blocking form of rounds 1-3 ("blocks until the frame is fused"). */
int mf_process_frame(mf_ctx* ctx, const uint8_t* rgb, const float* depth, const uint8_t* mask,
                     const int32_t* class_ids, int32_t n_masks, int64_t timestamp, const float* in_pose16,
                     float weight_multiplier, int32_t bootstrap);
/* Same, inputs already resident in HBM (device pointers); enqueues the whole frame on the context's stream and
 * returns without waiting.  mf_sync() (or any getter) waits. */
int mf_process_frame_dev(mf_ctx* ctx, const uint8_t* d_rgb, const float* d_depth, const uint8_t* d_mask,
                         int64_t timestamp, float weight_multiplier);
/* FrameData::classIDs (Core/FrameData.h:25-48) of the masks handed to mf_process_frame_dev: class_ids[v] = class of mask value v
 * (n <= 256; until it is called every mask value is class 0) */
int mf_set_mask_class_ids(mf_ctx* ctx, const int32_t* class_ids, int32_t n);
/* Waits for everything enqueued on the context's stream.  MF_EHIP (text in mf_last_error) for a HIP failure, and when the ordered compaction
 * of a full map's Model::clean gave up one of its bounded waits (never in a correct run; that model's map is then not valid). */
int mf_sync(mf_ctx* ctx);

/* MaskFusion::setTick (Core/MaskFusion.h:206); only after the first frame (tick 1 initialises the map) */
int mf_set_tick(mf_ctx* ctx, int32_t tick);
/* MaskFusion::preallocateModels (Core/MaskFusion.h:57, Core/MaskFusion.cpp:144-149) */
int mf_preallocate_models(mf_ctx* ctx, uint32_t count);
/* MaskFusion::predict (Core/MaskFusion.h:76) */
int mf_predict(mf_ctx* ctx);

/* MaskFusion::getTick / getModels().size() / Model::getPose / lastCount / getConfidenceThreshold
 * (Core/MaskFusion.h:88-90,194; Core/Model/Model.h:180,233).  `model` is the index in the model list (0 = background,
 * objects in spawn order, MaskFusion::getModels()); mf_model_info gives the Model::getID() behind an index. */
int mf_get_tick(mf_ctx* ctx, int32_t* tick);
int mf_num_models(mf_ctx* ctx, int32_t* n);
int mf_get_pose(mf_ctx* ctx, int32_t model, float* out_pose16);
int mf_get_surfel_count(mf_ctx* ctx, int32_t model, uint32_t* count);
/* Asynchronous device-side copy of a model's state into a caller-owned DEVICE buffer of 16 floats
 * {R row-major (9), t (3), lastICPError, lastICPCount, surfel count, alive}: what the multi-GPU gather ships per rank
 * (the reference logs the same per model, Core/MaskFusion.cpp:580-602) without a host round trip. */
int mf_model_state_dev(mf_ctx* ctx, int32_t model, float* d_out16);
/* the same for every model of the list in one call: d_out16[16 * i ..] = models[i]; capacity = models the buffer holds */
int mf_models_state_dev(mf_ctx* ctx, float* d_out16, int32_t capacity);
/* ids of the model list (MaskFusion::models, Core/MaskFusion.h:329-333) in list order; host state, no synchronisation */
int mf_get_model_ids(mf_ctx* ctx, int32_t* ids, int32_t capacity, int32_t* n);
/* Model::getPoseLog (Core/Model/Model.h:257-262) of model i, chronological: ts[e] = the frame's timestamp, p7[e] =
 * {tx ty tz qx qy qz qw} of cam->world (background) or obj->world (objects), Core/MaskFusion.cpp:580-596.
 * ts/p7 may be NULL to query *count only. */
int mf_get_pose_log(mf_ctx* ctx, int32_t model, int64_t* ts, float* p7, uint32_t max_entries, uint32_t* count);
/* MaskFusion::exportPoses (Core/MaskFusion.cpp:851-879): writes <export_dir>poses-<id>.txt ("ts[s] tx ty tz qx qy qz qw",
 * 6 decimals; ts = timestamp * 1e-6) for every live and dropped model */
int mf_export_poses(mf_ctx* ctx, const char* export_dir);
/* MaskFusion::savePly (Core/MaskFusion.cpp:733-849): writes <export_dir>cloud-<id>.ply per live model */
int mf_save_ply(mf_ctx* ctx, const char* export_dir);
/* {lastICPError, lastICPCount, lastRGBError, lastRGBCount, lastSO3Error, lastSO3Count, so3 iterations, rejected by the
 * 0.3 m rule} of the last tracking step of model i (RGBDOdometry.h:68-75, RGBDOdometry.cpp:477-481) */
int mf_get_track_stats(mf_ctx* ctx, int32_t model, float* out8);
/* No upstream twin.  The device solves the 6x6 Gauss-Newton system (RGBDOdometry.cpp:447-459 hands it to Eigen::LDLT, diagonal pivoting, on
 * float-rounded sums) with an unpivoted LDL^T on fp64 sums: identical to rounding for a well-posed system, NOT for a rank-deficient one
 * (DESIGN.md finding F4).  *ill_iterations = how many iterations of the model's last geometric tracking step were outside that domain:
 * fewer than 6 inliers, or smallest pivot < 1e-8 x largest diagonal entry (=> cond(A) > 1e8).  0 means the step is the reference's to rounding. */
int mf_get_gn_condition(mf_ctx* ctx, int32_t model, int32_t* ill_iterations);
/* RGBDOdometry::lastICPError / lastICPCount (Core/Utils/RGBDOdometry.h) of `model` */
int mf_get_icp_stats(mf_ctx* ctx, int32_t model, float* last_error, float* last_count);
/* Model::downloadMap (Core/Model/Model.h:206, Model.cpp:943-974): out has room for max_count*12 floats */
int mf_download_map(mf_ctx* ctx, int32_t model, float* out, uint32_t max_count, uint32_t* count);
/* Model::getID / getClassID / lastCount / getConfidenceThreshold / isNonstatic (Core/Model/Model.h:180,241-268) */
typedef struct mf_model_info_t {
    int32_t id, class_id;
    uint32_t surfels;
    float confidence_threshold;
    int32_t is_static;
    uint32_t age;
} mf_model_info_t;
int mf_model_info(mf_ctx* ctx, int32_t model, mf_model_info_t* out);
/* SegmentationResult::fullSegmentation of the last frame (Core/Segmentation/SegmentationResult.h:35): H*W model ids,
 * 255 = ignored.  Only meaningful with enable_multiple_models. */
int mf_download_segmentation(mf_ctx* ctx, uint8_t* out);
/* The exportSegmentation branch of processFrame (Core/MaskFusion.cpp:299-303): the label image of the last frame with 255 (ignored)
 * zeroed, as an 8-bit greyscale PNG at `path` (upstream: exportDir + "Segmentation<tick>.png") */
int mf_export_segmentation_png(mf_ctx* ctx, const char* path);
/* The cv::imwrite(<name>.png, CV_8UC1) of that branch on its own: H*W bytes -> 8-bit greyscale PNG.  HOST pointer, no GPU involved. */
int mf_write_png_gray8(const char* path, const uint8_t* img, int32_t width, int32_t height);
/* Headless rendering of the surfel maps (Model::renderPointCloud as MainController::drawScene calls it, Core/Model/Model.cpp:287-346,
 * GUI/MainController.cpp:609-720): every drawn surfel is the disc of radius nr.w around its position, in the plane normal to nr.xyz, seen
 * from a virtual pinhole camera; a pixel is covered where the ray through its centre meets the disc, the smaller camera z wins (ties: the
 * surfel drawn first -- the background, then the objects in list order, buffer order within a model).  Vertex test: confidence above the
 * model's threshold, or draw_unstable.  Colour types (MainController.h:38): 1 normals, 2 colour, 3 times (also unstable surfels unless the
 * type is 1 or 2), 4 labels (palette[classID mod n] x max(|n.(1,1,1)|, 0.8); the background in grey), anything else grey; draw_window
 * darkens surfels not seen within timeDelta by 0.25; channels are round(clamp(c, 0, 1) 255).  draw_points: a confident surfel covers the
 * pixel its centre projects into (types 1, 2, else grey).  DESIGN.md "Rendering" has the whole restatement and the deviations.
 * The render reads the models and changes nothing (no compaction, run table, bounding box, timing slot or visibility cache). */
typedef struct mf_render_view_t {
    int32_t width, height;                      /* 1 .. 4096 each */
    float fx, fy, cx, cy;
    float near_z, far_z;                        /* fragments outside [near_z, far_z] of camera z are dropped; 0 < near_z < far_z */
    float pose16[16];                           /* camera -> world, column-major (mf_get_pose's layout); camera x right, y down, z forward */
    int32_t background_color_type, object_color_type;
    int32_t draw_unstable, draw_points, draw_window, draw_background, draw_objects;
    uint8_t clear_rgba[4];                      /* pixels no surfel covers (the GUI clears to white) */
    uint64_t model_mask;                        /* 0: every model draw_background / draw_objects allow; else bit i = model list index i (< 64) */
    int32_t reserved[8];                        /* zero */
} mf_render_view_t;
/* The GUI's follow-pose view (MainController.cpp:610-640, GUI.h:73,198-211): the current camera pose moved 0.2 m back along its optical
 * axis, fx = fy = 420, the principal point at the image centre, near 0.1, far 1000, colour types 2, the background and the objects drawn,
 * cleared to white.  icl != 0 rolls the view by 180 degrees about its axis (upstream's up vector for ICL-NUIM). */
int mf_default_render_view(mf_ctx* ctx, int32_t width, int32_t height, int32_t icl, mf_render_view_t* out);
/* The view of the frame just processed, for comparing a render with that frame (mf_view_score_dev): the context's image size and
 * intrinsics, the current camera pose itself (the one mf_default_render_view starts from, not moved back), near 0.01, far 1000, colour
 * types 2, the background and the objects drawn, draw_unstable 0, cleared to opaque black. */
int mf_sensor_render_view(mf_ctx* ctx, mf_render_view_t* out);
/* The library's own label palette: n = min(capacity, 64) RGB triples in [0, 1] -> out (out may be NULL to query *n = 64). */
int mf_default_palette(float* out_rgb, int32_t capacity, int32_t* n);
/* Renders `view` into out_rgba (H*W*4 bytes, row-major; HOST pointer), optionally the camera z of every pixel (0 where nothing is drawn) and
 * the model list index that drew it (-1: none).  palette: n_palette RGB triples for colour type 4 (class ids index it modulo n_palette;
 * palette NULL with n_palette 0: the library's palette).  MF_EINVAL (mf_last_error says why) for a bad size, a null output, a model mask
 * naming a model that does not exist, an empty palette with type 4.  Synchronous. */
int mf_render_view(mf_ctx* ctx, const mf_render_view_t* view, const float* palette, int32_t n_palette, uint8_t* out_rgba,
                   float* out_depth, int32_t* out_model);
/* The same with DEVICE outputs, enqueued on mf_get_stream(ctx) without waiting. */
int mf_render_view_dev(mf_ctx* ctx, const mf_render_view_t* view, const float* palette, int32_t n_palette, uint8_t* d_out_rgba,
                       float* d_out_depth, int32_t* d_out_model);
/* Run evaluation: fixed-radius nearest neighbour from every query point to a target cloud, on the GPU (kernels: mf_eval.hip; DESIGN.md
 * "Cloud evaluation").  For query i, the target j with the smallest fp32 d2 = dx*dx + dy*dy + dz*dz (d = query - target, evaluated in that
 * order without contraction) among the finite targets with d2 <= fl(radius * radius); ties go to the smallest j.  d_dist[i] = sqrtf(d2),
 * d_idx[i] = j; +inf and -1 when no target is in range or the query is not finite.  The result is bit-identical to an fp32 brute force and
 * the same for every call.  Targets are read as x, y, z at d_target + j * target_stride floats (3: xyz, 4: float4, 12: mf_download_map's
 * records), queries likewise; query_to_target16 (HOST, column-major 4 x 4, or NULL) maps each query first: x' = ((T00 x + T01 y) + T02 z)
 * + T03 in fp32.  MF_EINVAL for a radius <= 0 or not finite, a stride < 3, more than 2^30 targets or queries, a null pointer, a workspace smaller
 * than mf_cloud_nn_workspace says or not 16-byte aligned, a transform that is not finite, and a finite coordinate (target, or query after
 * the transform) with |x / radius| >= 2^30.  Enqueued on `stream`, which the call synchronises before it returns (to report the last case). */
int mf_cloud_nn_workspace(int64_t n_target, uint64_t* bytes);   /* device workspace bytes mf_cloud_nn_dev needs for n_target targets */
int mf_cloud_nn_dev(const float* d_target, int32_t target_stride, int64_t n_target, const float* d_query, int32_t query_stride, int64_t n_query,
                    const float* query_to_target16, float radius, float* d_dist, int32_t* d_idx, void* d_workspace, uint64_t workspace_bytes,
                    void* stream);
/* The same against the live map of `model`, read where it lies: its surfels with confidence > conf_threshold are the targets (the model's own
 * threshold selects what mf_save_ply writes), and d_idx indexes the array mf_download_map returns for the model.  query_to_model16 (HOST or
 * NULL) maps the queries into the model's frame.  Runs on mf_get_stream(ctx) with a workspace the context owns and grows on demand; writes
 * no model state (frames processed afterwards are bit-identical to frames processed without the call).  Synchronous. */
int mf_model_cloud_nn_dev(mf_ctx* ctx, int32_t model, float conf_threshold, const float* d_query, int32_t query_stride, int64_t n_query,
                          const float* query_to_model16, float radius, float* d_dist, int32_t* d_idx);
/* Rigid registration of a query cloud onto a target cloud, one Gauss-Newton step at a time (kernels: mf_eval.hip; DESIGN.md "Cloud
 * registration"; the loop around it: maskfusion_amd.eval.register).  mf_cloud_icp_build_dev builds mf_cloud_nn_dev's grid for `radius` once, into a
 * workspace of mf_cloud_icp_workspace(n_target, n_query) bytes (16-byte aligned) that the steps then read; it keeps every target's position and,
 * with normal_offset >= 3 (floats from the start of the target's record, normal_offset + 3 <= target_stride), its normal, which is used as given
 * and expected to have unit length.  normal_offset < 0: no normals, the steps are point-to-point.  A target whose position or normal is not finite
 * is skipped.  mf_cloud_icp_step_dev maps every query by query_to_target16 and pairs it with a target exactly as mf_cloud_nn_dev does (the same
 * fp32 transform, distance, radius test and tie rule: the pairs are those of mf_cloud_nn_dev on the same inputs), then sums, in fp64 from the
 * fp32 x', the target p and the normal n:  point-to-plane  r = n . (x' - p),  J = [n, x' x n];  point-to-point the three rows of [I, -[x']x]
 * with r = x' - p.  d_out29 (DEVICE, 29 doubles) = for i = 0..5: (J^T J)[i][i..5], (J^T r)[i]; then sum r^2; then the number of pairs -- the
 * layout of mf_k_gn_solve's sys29.  The update x = (t, w) solves J^T J x = -J^T r and composes as T <- [exp(w) | t] T.  The sums use no
 * floating-point atomics and do not depend on the order of execution: the same inputs give the same 29 doubles bit for bit.  The step writes
 * only the workspace and d_out29.  MF_EINVAL as for mf_cloud_nn_dev, and for a normal_offset of 0..2 or beyond the stride, a workspace no build
 * has filled or one smaller than mf_cloud_icp_workspace says for n_query.  Both calls are enqueued on `stream` and synchronise it before they return.
 * (Against a live model: mf_download_map first; its records carry the normal at offset 8.) */
int mf_cloud_icp_workspace(int64_t n_target, int64_t n_query, uint64_t* bytes);
int mf_cloud_icp_build_dev(const float* d_target, int32_t target_stride, int32_t normal_offset, int64_t n_target, float radius,
                           void* d_workspace, uint64_t workspace_bytes, void* stream);
int mf_cloud_icp_step_dev(void* d_workspace, uint64_t workspace_bytes, const float* d_query, int32_t query_stride, int64_t n_query,
                          const float* query_to_target16, double* d_out29, void* stream);
/* Normals of a point cloud from its own radius neighbourhoods, on the GPU (kernels: mf_eval.hip; DESIGN.md "Cloud normals"): what a cloud
 * without nx / ny / nz needs before it can be the target of a point-to-plane registration.  Points are read as x, y, z at d_points + i * stride
 * floats.  The neighbours of point i are the finite points j, i itself included, whose fp32 d2 = dx*dx + dy*dy + dz*dz (d = p_j - p_i, without
 * contraction) passes d2 <= fl(radius * radius): mf_cloud_nn_dev's radius test, over mf_cloud_nn_dev's grid.  d_count[i] = k, their number
 * (exact).  With d in fp64 and every sum in fp64: m = sum d / k, C = sum d d^T / k - m m^T; C is decomposed by cyclic Jacobi rotations in fp64
 * (a fixed number of sweeps) into l0 <= l1 <= l2.  d_normals[i] = (the unit eigenvector of l0, the surface variation l0 / (l0 + l1 + l2)).
 * Sign: with viewpoint3 (HOST, 3 floats: v) the normal faces it, n . (v - p_i) >= 0; with NULL, or where that product is exactly 0, the
 * component of largest magnitude is positive (ties: the lowest axis).  No normal -- NaN in all four lanes, d_count[i] still k -- for a point
 * that is not finite (k = 0), for k < min_neighbours, and for l1 <= 1e-12 l2: neighbours on one line or in one place (twelve digits lie
 * between that and both the rounding of C and any sampled surface).  A bucket of the grid holds its points in the order of the build's atomics,
 * so the fp64 sums and the normal are reproducible to rounding only (about k 2^-53 over the relative gap of the eigenvalues between two calls);
 * d_count is the same for every call.  MF_EINVAL as for mf_cloud_nn_dev (radius, stride, more than 2^30 points, a null pointer, the workspace
 * -- mf_cloud_normals_workspace(n) bytes, 16-byte aligned --, a finite coordinate with |x / radius| >= 2^30), and for min_neighbours < 3 or a
 * viewpoint that is not finite.  Enqueued on `stream`, which the call synchronises before it returns. */
int mf_cloud_normals_workspace(int64_t n, uint64_t* bytes);
int mf_cloud_normals_dev(const float* d_points, int32_t stride, int64_t n, float radius, int32_t min_neighbours, const float* viewpoint3,
                         float* d_normals /* [n][4] */, int32_t* d_count /* [n] */, void* d_workspace, uint64_t workspace_bytes, void* stream);
/* FPFH descriptors of a cloud with normals, on the GPU (kernels: mf_eval.hip; DESIGN.md "Global registration"): what a registration without a
 * starting pose matches (maskfusion_amd.eval.register_global).  Points are read as x, y, z and, at normal_offset, nx, ny, nz at
 * d_points + i * stride floats.  A point is ELIGIBLE when its position and its normal are finite and the normal is not zero; normals are
 * normalised in fp64 first.  The neighbours N(i) of an eligible i are the eligible j != i whose fp32 d2 passes d2 <= fl(radius * radius):
 * mf_cloud_nn_dev's test over mf_cloud_nn_dev's grid.  Pair features, in fp64 from the fp32 inputs: d = p_j - p_i, L = |d| (L == 0: the
 * pair is not counted); a1 = n_i . d / L, a2 = n_j . d / L; if |a1| < |a2| then n1 = n_j, n2 = n_i, d <- -d, f3 = -a2, else n1 = n_i,
 * n2 = n_j, f3 = a1; v = d x n1 (|v| == 0: not counted), v <- v / |v|, w = n1 x v; f2 = v . n2, f1 = atan2(w . n2, n1 . n2).  Bins, clamped
 * to 0..10: b1 = floor(11 (f1 + pi) / (2 pi)), b2 = floor(11 (f2 + 1) / 2), b3 = floor(11 (f3 + 1) / 2).  SPFH_i = the 33 counts
 * (b1 | 11 + b2 | 22 + b3) over N(i), k_i = the number of counted pairs: d_spfh[i] = (33 counts, k_i), exact and the same for every call;
 * d_spfh may be NULL.  FPFH_i[b] = sum over j in N(i) with L_ij > 0 and k_j > 0 of (1 / L_ij^2) SPFH_j[b] / k_j, summed in fp64 -- the
 * point's own SPFH is not added: PCL's FPFHEstimation --, each of the three 11-bin parts scaled to the sum 100 and stored as fp32 in
 * d_fpfh[i].  A row is NaN, all 33 values, for a point that is not eligible or when a part sums to 0.  The sums follow the order of the
 * build's atomics: d_fpfh is reproducible to the last fp64 bits before the fp32 store.  MF_EINVAL as for mf_cloud_normals_dev (radius,
 * more than 2^30 points, a null pointer, the workspace -- mf_cloud_fpfh_workspace(n) bytes, 16-byte aligned --, an eligible point with
 * |x / radius| >= 2^30), and for a normal_offset below 3 or a normal that ends beyond the stride.  Enqueued on `stream`, which the call
 * synchronises before it returns. */
int mf_cloud_fpfh_workspace(int64_t n, uint64_t* bytes);
int mf_cloud_fpfh_dev(const float* d_points, int32_t stride, int32_t normal_offset, int64_t n, float radius, float* d_fpfh /* [n][33] */,
                      int32_t* d_spfh /* [n][34] or NULL */, void* d_workspace, uint64_t workspace_bytes, void* stream);
/* The nearest descriptor by brute force, on the GPU (kernel: mf_eval.hip).  d_target [n_target][dim], d_query [n_query][dim], DEVICE fp32,
 * dim 1..64.  d_idx[i] = the target j with the smallest fp32 d2 = sum over the bins b = 0 .. dim - 1, in that order, of (q_b - t_b)^2,
 * every operation rounded on its own; ties go to the smallest j; d_d2[i] = that d2.  A row with a NaN is nobody's match, and a query with a
 * NaN (or no target) gets -1 and +inf.  The result is a function of the inputs alone.  MF_EINVAL for a dim outside 1..64, more than 2^30
 * rows or a null pointer.  Enqueued on `stream`, which the call synchronises before it returns. */
int mf_feature_match_dev(const float* d_target, int64_t n_target, const float* d_query, int64_t n_query, int32_t dim, int32_t* d_idx,
                         float* d_d2, void* stream);
/* The hypothesis search of a registration without a start, on the GPU (kernels: mf_register.hip; DESIGN.md "Inactive models and re-detection";
 * the Python side: maskfusion_amd.eval.ransac_correspondences(device=True)).  src[k] <-> dst[k], k = 0 .. m - 1, are correspondences: x y z
 * at d_src + k * stride and d_dst + k * stride floats, DEVICE fp32, stride >= 3; the pose sought maps src onto dst.  d_triples holds h
 * triples (i0, i1, i2) of correspondence indices, DEVICE int32.  Everything below is computed in fp64 from the fp32 values, every operation
 * rounded on its own (no contraction), in the order written; s0 s1 s2 are the triple's points in src, d0 d1 d2 in dst.
 * STATUS of a triple, the first that applies:
 *   1  an index is outside [0, m), or two indices are equal;
 *   3  one of the six points has a coordinate that is not finite;
 *   2  the edge test fails.  For the pairs (0,1), (0,2), (1,2) in that order, with (dx, dy, dz) the difference of the pair's points:
 *      ls = sqrt((dx*dx + dy*dy) + dz*dz) in src, ld likewise in dst; the pair passes when min(ls, ld) > 0 and
 *      min(ls, ld) >= (1.0 - edge_tolerance) * max(ls, ld), the factor formed once on the host (a rigid motion keeps lengths: the rule of
 *      maskfusion_amd.eval.ransac_correspondences);
 *   3  degenerate: with a = s1 - s0, b = s2 - s0, w = a x b = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx) and
 *      |w| = sqrt((wx*wx + wy*wy) + wz*wz): |w| == 0 in src or in dst;
 *   0  tested.
 * FIT of a tested triple.  Closed form from the triple's two frames -- NOT Horn's least-squares rule (no SVD: a device SVD could not be
 * restated bit for bit); it maps s0, s1, s2 onto d0, d1, d2 exactly only when the triangles are congruent, which the edge test asks for up to
 * its tolerance.  In src: e1 = a / |a| (|a| as ls above, per component), e3 = w / |w|, e2 = e3 x e1 (the cross product as above); in dst f1, f2,
 * f3 likewise.  R[r][c] = (f1[r]*e1[c] + f2[r]*e2[c]) + f3[r]*e3[c].  cs = ((s0 + s1) + s2) / 3.0 per component, cd likewise.
 * t[r] = cd[r] - ((R[r][0]*cs.x + R[r][1]*cs.y) + R[r][2]*cs.z).
 * SCORE.  For every k: q[r] = ((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + t[r] of src[k], (dx, dy, dz) = q - dst[k], e2 = (dx*dx + dy*dy) + dz*dz;
 * k is an INLIER iff e2 <= inlier_distance * inlier_distance, the product formed once on the host in fp64.  A correspondence with a NaN
 * fails the comparison: it is never an inlier.
 * OUTPUT, all DEVICE.  d_status[j]: the status.  d_counts[j]: the number of inliers of a tested triple, 0 for the others.  d_best = {j*, count}:
 * the tested triple with the largest count, ties to the smallest index, or {-1, 0} when no triple is tested.  d_inlier[k] (may be NULL): 1 for
 * the inliers under j*'s pose, all 0 when j* = -1.  d_pose (may be NULL): j*'s 12 doubles R[0][0] R[0][1] R[0][2] t[0], R[1][0] ..., untouched
 * when j* = -1.  Every decision is an integer count or an index: the result is a function of the inputs alone and the same for every call.
 * The re-fit on the winner's inliers (Horn's rule) is the caller's, on the host.
 * MF_EINVAL, with nothing enqueued and nothing written: a null d_src, d_dst, d_triples, d_counts, d_status or d_best when m > 0 and h > 0;
 * stride < 3; m or h negative or above 2^24; inlier_distance not finite or <= 0; edge_tolerance outside [0, 1).  m < 3 or h == 0 is MF_OK
 * with d_best = {-1, 0}.  Needs no context and no workspace.  Enqueued on `stream` (a memset and up to three launches); the call does NOT
 * wait: synchronise the stream before reading the outputs. */
int mf_pose_ransac_dev(const float* d_src, const float* d_dst, int32_t stride, int32_t m, const int32_t* d_triples /* [h][3] */, int32_t h,
                       double inlier_distance, double edge_tolerance, uint32_t* d_counts /* [h] */, uint8_t* d_status /* [h] */,
                       int32_t* d_best /* [2]: index or -1, count */, uint8_t* d_inlier /* [m] or NULL */, double* d_pose /* [12] or NULL */,
                       void* stream);
/* Map-to-map fusion, on the GPU (kernels: mf_merge.hip; DESIGN.md "Map merging"; the Python side: maskfusion_amd.merge): the surfels of a
 * source map, moved by a rigid transform, are merged into a target map by the weighted rule of the frame fusion (Core/Shaders/update.vert:64-93)
 * or appended to it.  No upstream twin: the reference fuses depth frames only.  d_target, d_source, d_out: DEVICE, 16-byte aligned, records of 12
 * floats in mf_download_map's layout {x y z conf | colour, unused, initTime, lastTime | nx ny nz radius}; d_out overlaps neither input.  All
 * arithmetic is fp32, rounded operation by operation in the order written (no contraction).
 * 1. TRANSFORM.  source_to_target16 (HOST, column-major 4 x 4, or NULL: nothing is applied) maps a source's position as mf_cloud_nn_dev maps a
 *    query, x' = ((T00 x + T01 y) + T02 z) + T03, and its normal by the same rows without the translation, n'x = (T00 nx + T01 ny) + T02 nz; the
 *    normal is not renormalised.  Confidence, colour, the unused word, both stamps and the radius pass through.
 * 2. ELIGIBILITY.  A source is DROPPED when a component of x' or n' is not finite, or when its confidence or its radius is not finite or is
 *    <= 0: d_match = -2, counted, nowhere in the output.  A target with a position or a normal that is not finite is never a partner; it is
 *    copied through unchanged.  Every other target is ELIGIBLE.
 * 3. PARTNER.  With d = x' - p and d2 = dx*dx + dy*dy + dz*dz (mf_cloud_nn_dev's expression and order), the candidates of a source are the
 *    eligible targets with d2 <= fl(radius * radius) AND (n'x qx + n'y qy) + n'z qz >= min_cos, q the target's normal.  The partner is the
 *    candidate with the smallest d2, ties to the smallest target index: the nearest target that passes the normal test, not the nearest target
 *    tested afterwards (a wall seen from both sides finds its own side).  d_match = its index, or -1 without a candidate.  Every source chooses
 *    against the INPUT targets, as a frame's association is made against the index map before update.vert runs.
 * 4. MERGE.  A target q receives the sources that chose it in ascending source index, each merged into the record the merge before it left.
 *    With c = q.conf and a = s.conf:  if s.radius < 1.5f * q.radius:  position ((c * v_k) + (a * v_g)) / (c + a) per component;  colour
 *    encode(((c * k) + (a * g)) / (c + a) per channel) of the two decoded colours (color_encoding.glsl: decode (float)(((int)colour >> 16, 8, 0)
 *    & 255) / 255.0f, encode (float)(((int)roundf(r * 255.0f) << 8) + (int)roundf(g * 255.0f) << 8) + (int)roundf(b * 255.0f)), roundf half away
 *    from zero; colours are expected in [0, 2^24));  {normal, radius} ((c * nr_k) + (a * nr_g)) / (c + a) per component, the normal then
 *    multiplied by 1.0f / sqrtf((x*x + y*y) + z*z).  In both branches conf = c + a and lastTime = s.lastTime > q.lastTime ? s.lastTime :
 *    q.lastTime; initTime and the unused word stay the target's.  (Which bit pattern a NaN has that this arithmetic PRODUCES, e.g. from an
 *    infinite confidence, is the hardware's; a NaN that is only carried keeps its bits.)
 * 5. OUTPUT.  d_out[0, n_target): the targets in their order, merged.  Behind them the unmatched eligible sources in ascending source index,
 *    as transformed.  *n_out (HOST) = n_target + appended.  stats4 (HOST) = {merges that averaged, merges that added the confidence only,
 *    appended, dropped}: the four add up to n_source.  d_match (DEVICE, [n_source], or NULL).  out_capacity < n_target + appended: MF_ENOMEM, *n_out
 *    the count needed, d_out untouched.
 * 6. MF_EINVAL as for mf_cloud_nn_dev -- a null pointer (n_out and stats4 included), more than 2^30 targets or sources, a radius <= 0 or not
 *    finite, a transform that is not finite, a workspace smaller than mf_cloud_merge_workspace says or not 16-byte aligned, a finite coordinate
 *    (eligible target, or eligible source after the transform) with |x / radius| >= 2^30 -- and for a min_cos that is not finite or outside
 *    [-1, 1], records that are not 16-byte aligned and a negative out_capacity; d_out is untouched then.  n_source == 0 (the targets are
 *    copied) and n_target == 0 (the eligible sources are appended) are valid.
 * Targets are found over mf_cloud_nn_dev's grid with cell edge `radius`.  A target's sources are put in order by an insertion sort, so the
 * time is quadratic in the length of ONE list -- the number of source surfels on one target surfel, a handful when two maps of similar
 * density meet; any length is correct.  Only integer atomics are used and nothing in the output depends on their order: the same inputs give
 * the same bytes on every call.  Enqueued on `stream`, which the call synchronises (once before d_out is written, once before it returns). */
int mf_cloud_merge_workspace(int64_t n_target, int64_t n_source, uint64_t* bytes);
int mf_cloud_merge_dev(const float* d_target /* [n_target][12] */, int64_t n_target, const float* d_source /* [n_source][12] */, int64_t n_source,
                       const float* source_to_target16, float radius, float min_cos, float* d_out /* [out_capacity][12] */, int64_t out_capacity,
                       int64_t* n_out, int32_t* d_match, uint64_t stats4[4], void* d_workspace, uint64_t workspace_bytes, void* stream);
/* A triangle mesh of a cloud of oriented points (surfels), on the GPU (kernels: mf_mesh.hip; DESIGN.md "Surfel meshing"; the Python side:
 * maskfusion_amd.mesh): naive surface nets over a moving-least-squares signed distance to the points' tangent planes.  No table of cases.
 * INPUT.  n records of `stride` floats at d_points: x y z at offset 0, a normal at normal_offset (>= 3) and, with color_offset >= 3, three
 * colour floats there, in any linear scale (color_offset < 0: no colour).  A point is ELIGIBLE when its position and its normal are finite and
 * the normal is not zero -- mf_cloud_fpfh_dev's rule --; normals are normalised in fp64.  The others take no part.
 * LATTICE (HOST parameters).  origin3, voxel > 0, dims3 = corners per axis (each >= 2), support with voxel <= support <= 8 voxel,
 * min_neighbours >= 1.  Corner (i, j, k) stands, per axis, at xf = (float)((double)origin + (double)i * (double)voxel).
 * CORNER.  Its neighbours are the eligible points that pass mf_cloud_nn_dev's fp32 radius test against xf with radius = support (d2 = dx*dx +
 * dy*dy + dz*dz without contraction, d2 <= fl(support * support)), found over mf_cloud_nn_dev's grid.  In fp64 from the fp32 values, with
 * d = xf - p, q = (d . d) * (1 / support^2) and w = max(1 - q, 0)^2:  W = sum w,  f = sum w (n . d) / W,  a = sum w n / W,  c = sum w colour / W
 * (n the unit normal).  The corner is VALID when it has >= min_neighbours neighbours and W > 0.  A valid corner is INSIDE when f < 0; f == 0
 * counts as outside.
 * CELL (i, j, k) has the corners (i + {0,1}, j + {0,1}, k + {0,1}).  It is ACTIVE when all eight are valid and they are not all on one side.
 * QUADS.  The lattice edge from corner c to c + e_a (a = 0, 1, 2; u = (a + 1) mod 3, w = (a + 2) mod 3) whose two ends are valid and on
 * different sides gives one quad when the four cells around it -- c, c - e_u, c - e_u - e_w, c - e_w -- are all active: the vertices of
 * those cells in that order when f(c) < 0, in the reverse order otherwise.  Seen from the outside (f > 0) every face is counter-clockwise.
 * VERTICES.  A cell carries a vertex iff it is active and a quad names it: there is no unreferenced vertex.  Its position is the mean, over
 * the cell's sign-changing edges -- the x-edges first, then y, then z; within axis a the edges at offsets (0,0), (1,0), (0,1), (1,1) along
 * (u, w) --, of xa + t (xb - xa) with t = fa / (fa - fb), in fp64 from the fp32 corner positions.  Its normal is the normalised mean of
 * a_a + t (a_b - a_a) over the same edges, or zero when that mean is zero; its colour the plain mean of c_a + t (c_b - c_a).  All are stored
 * as fp32.
 * REPRODUCIBILITY.  The order of the vertices and of the quads is a function of the inputs alone (integer scans; no atomic's rank enters).
 * The fp64 sums of a corner follow the grid's bucket order, i.e. the order of the build's atomics, so positions, normals and colours are
 * reproducible to rounding only, as mf_cloud_normals_dev's normals are.
 * CALLS.  mf_cloud_mesh_build_dev does all the work but the output: *out receives a handle that owns its device memory (as a context does;
 * it keeps no pointer to d_points), *n_vertices and *n_quads the counts.  Memory and work follow the occupied part of the lattice, not its
 * volume, except for a directory of 4 bytes per block of 8 x 8 x 8 corners.  stage_ms (HOST, MF_MESH_STAGES floats, or NULL): the device
 * time of the stages in milliseconds -- 0 eligible points, normals and block marks, directory scan; 1 grid build; 2 the host's wait, read-back
 * and allocation; 3 block list and the field; 4 cells and quads; 5 the two scans.  Enqueued on `stream`, which the call synchronises before
 * it returns the counts.  n == 0 gives an empty mesh and MF_OK.  mf_cloud_mesh_emit_dev fills the caller's DEVICE arrays: d_vertices
 * [n_vertices][3], d_normals [n_vertices][3] or NULL, d_colors [n_vertices][3] or NULL (only for a mesh built with colour), d_cells
 * (int32 [n_vertices][3]: each vertex's lattice cell) or NULL, d_quads (int32 [n_quads][4]: vertex indices); it synchronises `stream` too.
 * mf_cloud_mesh_free releases the handle (NULL: nothing).
 * MF_EINVAL, with nothing enqueued and the reason in mf_last_error(NULL) (per thread), for a null pointer, n < 0 or n > 2^30, stride < 6, a
 * normal or colour offset below 3 or ending beyond the stride, an origin, voxel or support that is not finite, voxel <= 0, support outside
 * voxel .. 8 voxel, min_neighbours < 1, a dims entry < 2, a lattice corner with |x / support| >= 2^30 - 2 and a lattice of more than 2^27
 * blocks (the directory's limit); after the grid build, for an eligible point with |x / support| >= 2^30.  MF_ENOMEM when an allocation
 * fails or more than 2^20 blocks are occupied. */
typedef struct mf_mesh mf_mesh;
#define MF_MESH_STAGES 6
int mf_cloud_mesh_build_dev(const float* d_points, int32_t stride, int32_t normal_offset, int32_t color_offset, int64_t n, const float* origin3,
                            float voxel, const int32_t* dims3, float support, int32_t min_neighbours, mf_mesh** out, uint32_t* n_vertices,
                            uint32_t* n_quads, float* stage_ms, void* stream);
int mf_cloud_mesh_emit_dev(const mf_mesh* mesh, float* d_vertices, float* d_normals, float* d_colors, int32_t* d_cells, int32_t* d_quads,
                           void* stream);
void mf_cloud_mesh_free(mf_mesh* mesh);
/* Scoring against a triangle mesh, on the GPU (kernels: mf_eval_trimesh.hip; DESIGN.md "Mesh evaluation"; the Python side:
 * maskfusion_amd.eval.TriMesh, compare_cloud_mesh): the exact distance from every query point to the nearest triangle within a radius, and a
 * deterministic area-uniform sampler of the mesh whose samples serve wherever a reference cloud is consumed.
 * INPUT.  n_vertices vertices, x y z at d_vertices + i * vertex_stride floats; n_triangles index triples at d_triangles (DEVICE, int32
 * [n_triangles][3]).  A triangle (a, b, c) is ELIGIBLE when its three indices are in [0, n_vertices), its nine coordinates are finite with
 * |x / cell| < 2^30, and the fp64 squared norm of n = (b - a) x (c - a) is > 0:  ab = b - a, ac = c - a per component in fp64 from the fp32
 * values, n = (ab.y ac.z - ab.z ac.y, ab.z ac.x - ab.x ac.z, ab.x ac.y - ab.y ac.x), |n|^2 = (n.x n.x + n.y n.y) + n.z n.z.  The other
 * triangles are skipped: never returned, never sampled.  They keep their index: returned indices are indices into the caller's array.
 * *n_eligible receives the number of eligible triangles.  cell is the edge of the search structure's cells; it decides speed only.
 * DISTANCE.  The query is mapped first by query_to_mesh16 (HOST, column-major 4 x 4, or NULL) with mf_cloud_nn_dev's fp32 transform, x' =
 * ((T00 x + T01 y) + T02 z) + T03.  Then everything is fp64 from the fp32 values, every operation rounded on its own (no contraction); a dot
 * product is u . v = (u.x v.x + u.y v.y) + u.z v.z.  The closest point of an eligible triangle to p follows Ericson, Real-Time Collision
 * Detection 5.1.5, with the tests in the book's order and the first that holds deciding:
 *   ab = b - a, ac = c - a, ap = p - a;  d1 = ab . ap, d2 = ac . ap
 *   1. d1 <= 0 and d2 <= 0:                                   closest = a                  (vertex region A)
 *   bp = p - b;  d3 = ab . bp, d4 = ac . bp
 *   2. d3 >= 0 and d4 <= d3:                                  closest = b                  (vertex region B)
 *   vc = d1 d4 - d3 d2
 *   3. vc <= 0 and d1 >= 0 and d3 <= 0:  v = d1 / (d1 - d3),  closest = a + v ab           (edge AB)
 *   cp = p - c;  d5 = ab . cp, d6 = ac . cp
 *   4. d6 >= 0 and d5 <= d6:                                  closest = c                  (vertex region C)
 *   vb = d5 d2 - d1 d6
 *   5. vb <= 0 and d2 >= 0 and d6 <= 0:  w = d2 / (d2 - d6),  closest = a + w ac           (edge AC)
 *   va = d3 d6 - d5 d4
 *   6. va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:  w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),  closest = b + w (c - b)   (edge BC)
 *   7. otherwise:  den = 1 / ((va + vb) + vc), v = vb den, w = vc den,  closest = (a + ab v) + ac w   (face)
 * and D2 = (e.x e.x + e.y e.y) + e.z e.z with e = p - closest.  A triangle COUNTS when D2 <= (double)radius * (double)radius.  The result is
 * the minimum over (D2, t) lexicographically among the counting triangles -- ties go to the smallest triangle index t --: d_dist[i] =
 * (float)sqrt(D2), d_tri[i] = t, d_closest[i] (float [n_query][3], or NULL) the fp32 rounding of the fp64 closest point.  When no triangle
 * counts or the query is not finite: +inf, -1 and NaN.  The result depends on the mesh, the query and the radius alone: not on cell, and it
 * is the same for every call.  Queries are read as x, y, z at d_query + i * query_stride floats.
 * SAMPLING.  Systematic along the cumulative area; what decides is integer.  Triangle t has u_t = llrint(0.5 * sqrt(|n|^2) * (double)density
 * * 256) units (a unit is 1 / 256 sample; density in samples per unit area; 0 units when not eligible), S is the exclusive scan of u in
 * triangle order and S_total its sum.  n_samples = S_total / 256 (integer division).  Sample k sits at unit 256 k + 128: its triangle is the t
 * with S[t] <= unit < S[t + 1].  Its barycentrics come from the R2 sequence in fp64: r1 = frac((k + 1) * 0.7548776662466927), r2 =
 * frac((k + 1) * 0.5698402909980532), frac(x) = x - floor(x); when r1 + r2 > 1 both are replaced by 1 - r.  The point is
 * (a + r1 (b - a)) + r2 (c - a) per component in fp64, stored as fp32; the normal is n / sqrt(|n|^2), stored as fp32.  Samples come in the order
 * of k, so their triangle indices never decrease.
 * CALLS.  mf_trimesh_build_dev builds the search structure: *out receives a handle that owns its device memory and keeps no pointer to the
 * caller's arrays.  mf_trimesh_sample_plan_dev computes u and S for a density and returns n_samples; mf_trimesh_sample_emit_dev writes the
 * samples of the handle's latest plan: d_points [n_samples][3], d_normals [n_samples][3] or NULL, d_tri (int32 [n_samples]) or NULL.  Every
 * call is enqueued on `stream` and synchronises it before it returns.  Zero triangles is valid: every query gets +inf and -1, and there are 0
 * samples.  mf_trimesh_free releases the handle (NULL: nothing).
 * MF_EINVAL, with nothing enqueued and the reason in mf_last_error(NULL) (per thread), for a null pointer where the count is not zero (or a
 * null handle or result pointer), a count above 2^30 or below 0, vertex_stride or query_stride < 3, a cell, radius or density that is not
 * finite or <= 0, radius > 16 cell, a transform that is not finite, mf_trimesh_sample_emit_dev before a plan, and S_total >= 2^32; after the
 * query kernel, for a finite query with |x / cell| >= 2^30 after the transform.  MF_ENOMEM when an allocation fails or the structure would
 * hold 2^32 (triangle, cell) pairs. */
typedef struct mf_trimesh mf_trimesh;
int mf_trimesh_build_dev(const float* d_vertices, int32_t vertex_stride, int64_t n_vertices, const int32_t* d_triangles, int64_t n_triangles,
                         float cell, mf_trimesh** out, uint32_t* n_eligible, void* stream);
int mf_trimesh_distance_dev(const mf_trimesh* mesh, const float* d_query, int32_t query_stride, int64_t n_query, const float* query_to_mesh16,
                            float radius, float* d_dist, int32_t* d_tri, float* d_closest, void* stream);
int mf_trimesh_sample_plan_dev(mf_trimesh* mesh, float density, uint64_t* n_samples, void* stream);
int mf_trimesh_sample_emit_dev(const mf_trimesh* mesh, float* d_points, float* d_normals, int32_t* d_tri, void* stream);
void mf_trimesh_free(mf_trimesh* mesh);
/* Ray casting against a triangle mesh, on the GPU (kernels: mf_trimesh_ray.hip; DESIGN.md "Mesh rendering"; the Python side:
 * maskfusion_amd.eval.TriMesh.raycast / render, maskfusion_amd.meshseq, the mesh command's --views): for every ray the first triangle of an
 * mf_trimesh handle it hits.  The reference never renders a mesh: the definition is this project's own.
 * RAYS.  mf_trimesh_raycast_dev reads ray i as x y z at d_origin + i * ray_stride and at d_dir + i * ray_stride floats (ray_stride >= 3).
 * ray_to_mesh16 (HOST, column-major 4 x 4, or NULL) maps the origin with mf_cloud_nn_dev's fp32 transform, o' = ((T00 x + T01 y) + T02 z) +
 * T03, and the direction with its linear part alone in the same operation order, d' = (T00 x + T01 y) + T02 z: no translation.  A ray is
 * VALID when its six mapped values are finite and the direction is not zero.  The direction need not be of unit length: t counts in
 * lengths of d'.  Which triangles are ELIGIBLE is what mf_trimesh_build_dev decided.
 * INTERSECTION.  Everything after the transform is fp64 from the fp32 values, every operation rounded on its own (no contraction): the
 * watertight test of Woop, Benthin and Wald (Journal of Computer Graphics Techniques 2 (1), 2013), written out.  With o, d the mapped ray:
 *   kz = the first axis in the order x, y, z with the largest |d|;  kx = (kz + 1) % 3, ky = (kx + 1) % 3;  when d[kz] < 0, kx and ky swap
 *   Sx = d[kx] / d[kz],  Sy = d[ky] / d[kz],  Sz = 1 / d[kz]
 *   for each vertex P of (a, b, c):  P' = P - o per component;  Px = P'[kx] - Sx P'[kz],  Py = P'[ky] - Sy P'[kz],  Pz = Sz P'[kz]
 *   U = Cx By - Cy Bx,  V = Ax Cy - Ay Cx,  W = Bx Ay - By Ax
 *   the triangle is missed when (U < 0 or V < 0 or W < 0) and (U > 0 or V > 0 or W > 0)
 *   det = (U + V) + W;  det == 0 is a miss
 *   T = (U Az + V Bz) + W Cz,  t = T / det
 * A triangle COUNTS when tmin <= t <= tmax, compared after (double) of the fp32 arguments; tmax may be +inf.  An edge's function is computed
 * from its two end points and the ray alone, so two triangles that share an edge see the same value: no ray slips between them.
 * RESULT.  The minimum over (t, index) lexicographically among the counting triangles -- ties go to the smallest triangle index --:
 * d_t[i] = (float)t, d_tri[i] = index, d_uv[i] (float [n_rays][2], or NULL) = ((float)(V / det), (float)(W / det)), the weights of b and c
 * (a's is 1 - u - v), d_front[i] (uint8 [n_rays], or NULL) = det > 0: the ray meets the side from which (a, b, c) is counter-clockwise.
 * When nothing counts or the ray is not valid: +inf, -1, NaN NaN and 0.  The result depends on the mesh, the ray, tmin and tmax alone: not
 * on cell, and it is the same for every call.
 * PINHOLE.  mf_trimesh_render_dev casts, for pixel (x, y) of a width x height image, the ray of camera-frame origin (0, 0, 0) and direction
 *   (((float)x - cx) * (1.f / fx),  ((float)y - cy) * (1.f / fy),  1)       in fp32, each operation rounded on its own
 * -- the expressions by which the pipeline's vertex map (k_vmap_nmap) back-projects a pixel of depth 1, so a rendered depth back-projects
 * onto the mesh --, mapped by mesh_from_cam16 (HOST, required) as above, through the same device function as the generic call.  The
 * camera-frame z of the direction being 1, t IS the depth: d_depth[y * width + x] = (float)t, and 0, the pipeline's "no measurement",
 * where nothing counts; d_tri, d_uv, d_front as above, in pixel order.
 * CALLS.  Both are enqueued on `stream` and synchronise it before they return.  A mesh of zero triangles is valid: every ray misses.
 * MF_EINVAL, with nothing enqueued and the reason in mf_last_error(NULL) (per thread), for a null handle, a null pointer where the count is
 * not zero (d_uv and d_front may be NULL), a count above 2^30 or below 0, ray_stride < 3, a transform that is not finite (or, for the
 * pinhole form, NULL), tmin not finite, tmax NaN or tmax < tmin, fx or fy not finite or 0, cx or cy not finite, a width or height below 1
 * or above 16 384, and a mesh whose triangles in the cell grid (those mf_trimesh_build_dev did not put on its list of wide ones) span more
 * than 2^15 cells on an axis, which bounds every ray's walk: build the mesh with a larger cell. */
int mf_trimesh_raycast_dev(const mf_trimesh* mesh, const float* d_origin, const float* d_dir, int32_t ray_stride, int64_t n_rays,
                           const float* ray_to_mesh16, float tmin, float tmax, float* d_t, int32_t* d_tri, float* d_uv, uint8_t* d_front,
                           void* stream);
int mf_trimesh_render_dev(const mf_trimesh* mesh, int32_t width, int32_t height, float fx, float fy, float cx, float cy,
                          const float* mesh_from_cam16, float tmin, float tmax, float* d_depth, int32_t* d_tri, float* d_uv, uint8_t* d_front,
                          void* stream);
/* Segmentation scores on the GPU (kernels: mf_eval_image.hip; DESIGN.md "Segmentation evaluation"; the metrics built on them:
 * maskfusion_amd.eval.seg_metrics).  Both calls compare two label streams d_est, d_gt (DEVICE, uint8 [n_frames][height][width], any byte
 * alignment).  lut_est and lut_gt (HOST, 256 entries each) map a raw label value to a compact class index < n_est (< n_gt), or to 255: void.
 * n_est and n_gt are 1..64; by the callers' convention class 0 is the background.  The tables are copied into the launch's argument block when
 * the call is made: the call adds no copy to the stream and the host arrays may be reused at once.  Both calls zero their output on `stream`,
 * enqueue one kernel on it and return without waiting; they need no context.  All counters are integers: the result is exact and the same
 * for every call.  MF_EINVAL, with nothing enqueued, for a null pointer, width, height or n_frames < 1 (or width * height > 2^30), n_est or
 * n_gt outside 1..64, a table entry that is neither below its n nor 255, a pair entry that is neither < n_est nor 255, a radius outside 0..16.
 *
 * mf_label_confusion_dev: d_counts (DEVICE, uint32 [n_frames][n_gt][n_est]): [f][g][e] = the pixels of frame f whose ground truth maps to g
 * and whose estimate maps to e.  A pixel that is void on either side is counted nowhere.
 *
 * mf_label_boundary_dev: pair (HOST, n_gt entries): the estimate class matched to ground-truth class g, or 255 for none (two g may name
 * the same class).  A pixel is a boundary pixel of class k in a label image when its label maps to k and at least one of its 4-neighbours
 * inside the image maps to something else, void included; the image border by itself makes no boundary and a void pixel is a boundary
 * pixel of nothing.  d_out (DEVICE, uint32 [n_frames][n_gt][4]) = {n_est_boundary, est_hit, n_gt_boundary, gt_hit}: for g with pair[g] = e,
 * n_est_boundary counts the boundary pixels of e in the estimate and est_hit those of them that have a boundary pixel of g in the ground
 * truth at dx^2 + dy^2 <= radius^2 (integers; radius 0: the same pixel); n_gt_boundary and gt_hit are the mirror image.  For g with
 * pair[g] = 255 the row is {0, 0, n_gt_boundary, 0}. */
int mf_label_confusion_dev(const uint8_t* d_est, const uint8_t* d_gt, int32_t n_frames, int32_t height, int32_t width, const uint8_t* lut_est,
                           int32_t n_est, const uint8_t* lut_gt, int32_t n_gt, uint32_t* d_counts, void* stream);
int mf_label_boundary_dev(const uint8_t* d_est, const uint8_t* d_gt, int32_t n_frames, int32_t height, int32_t width, const uint8_t* lut_est,
                          int32_t n_est, const uint8_t* lut_gt, int32_t n_gt, const uint8_t* pair, int32_t radius, uint32_t* d_out, void* stream);
/* View scores on the GPU (kernel: mf_eval_image.hip; DESIGN.md "View evaluation"; the metrics built on them: maskfusion_amd.eval.view_metrics):
 * a render of the map from the camera that saw a frame -- mf_render_view_dev's colour and camera z from mf_sensor_render_view -- compared
 * with that frame.  d_render_rgba (DEVICE, uint8 [n_frames][height][width][4]; channel 3 is not read) and d_render_depth (DEVICE, float, same
 * frames) are the render, d_rgb (DEVICE, uint8 [n_frames][height][width][3]) and d_depth (DEVICE, float, metres) the input; the uint8 inputs
 * may have any byte alignment.  d_group (DEVICE, uint8 per pixel, or NULL: every pixel in group 0) names the group a pixel is counted in;
 * a pixel whose group is >= n_groups (1..64) is void: counted nowhere, but still read by its neighbours' windows.  The call follows the
 * label calls: it needs no context, zeroes d_counts on `stream`, enqueues one kernel and returns without waiting.  Every counter is an
 * integer: the result is exact and the same for every call.
 * A pixel is COVERED when its render depth is finite and > 0, DEPTH-VALID when its input depth is finite, > 0 and <= max_depth.
 * d_counts (DEVICE, uint64 [n_frames][n_groups][10]), per frame and group:
 *   0 pixels;  1 covered pixels;  2 depth-valid pixels;  3 pixels both covered and depth-valid ("pairs");
 *   4 pairs with |dz| <= tau, dz = render - input being one fp32 subtraction;
 *   5 the sum over the pairs of llrint((double)|dz| * 2^24) (|dz| below 2^38 m);
 *   6 the sum over the pixels of the squared byte differences of R, G and B (render channels 0..2 against input channels 0..2);
 *   7 the same sum over the covered pixels;
 *   8 SSIM pixels: those whose 11 x 11 window lies wholly inside the image;
 *   9 the sum over the SSIM pixels of llrint(s * 2^24) as a two's-complement int64, s = (s_R + s_G + s_B) / 3.0 being the mean of the
 *     three channels' SSIM values.
 * The uncovered pixels of the render take part in 6 and 9 with whatever the render holds there (its clear colour): a hole is an error.
 * SSIM of one channel at one pixel, in fp64 with every operation rounded on its own: the weights are g[k] = exp(-(k - 5)^2 / 4.5),
 * w[k] = g[k] / (g[0] + ... + g[10]), summed left to right (computed by the host, passed by value).  With x the render byte and y the input byte as
 * doubles, each of x, y, x x, x y, y y is filtered along the row (acc = 0; for k = 0..10: acc = acc + w[k] * q[col - 5 + k]) and the row results the
 * same way along the column, giving mx, my, Exx, Exy, Eyy.  vx = Exx - mx mx, vy = Eyy - my my, cxy = Exy - mx my and
 * s = ((2 mx my + C1) (2 cxy + C2)) / ((mx mx + my my + C1) (vx + vy + C2)) with C1 = 6.5025, C2 = 58.5225 ((0.01 255)^2, (0.03 255)^2).
 * Nothing is clamped.  MF_EINVAL, with nothing enqueued, for a null pointer other than d_group, width, height or n_frames < 1, width * height
 * > 2^24, n_groups outside 1..64, a max_depth that is not positive (FLT_MAX, "no limit", is accepted), a tau that is negative or not finite. */
int mf_view_score_dev(const uint8_t* d_render_rgba, const float* d_render_depth, const uint8_t* d_rgb, const float* d_depth,
                      const uint8_t* d_group, int32_t n_frames, int32_t height, int32_t width, int32_t n_groups, float max_depth, float tau,
                      uint64_t* d_counts, void* stream);
/* Cloud visibility on the GPU (kernel: mf_eval_visibility.hip; DESIGN.md "Cloud visibility"; what is built on it: maskfusion_amd.eval.Visibility,
 * observed): every point of a cloud classified against every depth frame of a sequence, so that a reference model can be culled to what the
 * sensor observed before completeness is taken over it.  Points are read as x, y, z at d_points + i * stride floats (3: xyz, 4: float4, 12:
 * mf_download_map's records).  d_depth (DEVICE, float [n_frames][height][width], metres) are the frames, d_cam_from_cloud (DEVICE, float
 * [n_frames][12]) the rows of each frame's 3 x 4 M, row-major, from the cloud's frame into the camera's.  The call follows the label and view
 * calls: it needs no context, validates the host arguments, enqueues one kernel on `stream` and returns without waiting; it reads the points,
 * the frames and the poses and writes only the two outputs.
 * Per point (x, y, z) and frame, in fp32 with every operation rounded on its own, in this order:
 *   xc = ((M00 x + M01 y) + M02 z) + M03, and yc, zc likewise from rows 1 and 2;
 *   IN FRONT: zc > near_z and zc <= far_z;
 *   u = fx * (xc / zc) + cx, v = fy * (yc / zc) + cy, col = floorf(u + 0.5f), row = floorf(v + 0.5f): the pixel centre is the integer coordinate;
 *   IN FRUSTUM: in front, 0 <= col < width and 0 <= row < height, compared as floats before any conversion: a NaN or an infinite coordinate
 *     fails every test, and a point that is not finite is in no frustum;
 *   d = depth[frame][row][col], VALID when it is finite and > 0; tol = tol_abs + tol_rel * d, dz = zc - d;
 *   an in-frustum point with a valid sample gets exactly one class: ON SURFACE |dz| <= tol; SEEN THROUGH dz < -tol (the sensor measured
 *     something farther along that pixel); OCCLUDED dz > tol.  An in-frustum point whose sample is not valid is a hole and gets no class.
 * d_counts (DEVICE, uint32 [n][4]) = {frames in frustum, on surface, seen through, occluded}; d_first (DEVICE, int32 [n]) = the smallest
 * frame_base + f with ON SURFACE, or -1.  accumulate == 0: both are overwritten (no zeroed buffer is needed).  accumulate != 0: the counts are
 * added to what is there, and d_first keeps a value >= 0 and is otherwise set: a sequence of any length can be streamed through in chunks of
 * frames with a running frame_base, and the result is the one call's.  All outputs are integers: the result is exact, independent of the
 * order of execution and the same for every call.  n == 0: MF_OK, nothing enqueued.  MF_EINVAL, with nothing enqueued and nothing written,
 * for a null pointer with n > 0, stride < 3, n < 0 or n > 2^30, n_frames, width or height < 1, width * height > 2^24, fx or fy not finite or
 * zero, cx or cy not finite, near_z not finite or <= 0, far_z <= near_z or NaN (FLT_MAX and +inf mean no limit), tol_abs or tol_rel negative or
 * not finite, frame_base < 0. */
int mf_cloud_visibility_dev(const float* d_points, int32_t stride, int64_t n, const float* d_depth, const float* d_cam_from_cloud,
                            int32_t n_frames, int32_t height, int32_t width, float fx, float fy, float cx, float cy, float near_z, float far_z,
                            float tol_abs, float tol_rel, int32_t frame_base, int32_t accumulate, uint32_t* d_counts /* [n][4] */,
                            int32_t* d_first /* [n] */, void* stream);
/* whether the last tracking step used the fill-in maps (MaskFusion::requiresFillIn, MaskFusion.cpp:630-648) */
int mf_get_last_fillin(mf_ctx* ctx, int32_t* used);

/* The parameters of a context, by key.  One table (maskfusion_amd/csrc/mf_params.inl) holds every key with its type, its legal values and who
 * may read and write it; the list below follows it row by row.  A flag stores value != 0 and reads back as 0 or 1; an int stores (int)value.
 * Every read-write key can be read back.  MF_EINVAL -- for an unknown key, a set of a read-only key, a get of a write-only key, a value outside
 * a key's legal values -- changes nothing and leaves "<key>: <reason>" in mf_last_error.
 *
 * Reference parameters: the per-frame setters of MaskFusion (Core/MaskFusion.h:132-182,234-263); their defaults are mf_config's.
 *   "depthCutoff", "icpWeight" (float)
 *   "confidenceThreshold" (float; the background's)
 *   "outlierCoefficient", "maxDepthProcessed" (float)
 *   "fastOdom", "so3" (int)
 *   "rgbOnly" (int; setRgbOnly: photometric term only)
 *   "pyramid", "timeDelta", "enableMultipleModels", "trackAllModels", "modelSpawnOffset" (int)
 *   "keepInactiveModels" (flag, 0): a dropped object model's map is archived on the inactive list (mf_inactive_count ...) when the rule of
 *     MaskFusion::inactivateModel (Core/MaskFusion.cpp:702) keeps it; 0: the map is deleted, and a drop costs no synchronisation
 *   "enableSmartModelDelete" (flag, 1), "modelKeepMinSurfels" (int, 4000), "modelKeepConfThreshold" (float, 0.3): upstream's members of those
 *     names (MaskFusion.h:398-399,414-415).  A model is kept iff !enableSmartModelDelete || (surfels >= modelKeepMinSurfels &&
 *     confidence threshold > modelKeepConfThreshold).  They matter only with "keepInactiveModels"
 *
 * Segmentation parameters:
 *   "newModelMinRelativeSize", "newModelMaxRelativeSize" (float; SegmentationPerformer.h:36-37)
 *   "mfThreshold", "mfWeightDistance", "mfWeightConvexity" (float), "mfMorphEdgeIterations", "mfMorphEdgeRadius", "mfMorphMaskIterations",
 *     "mfMorphMaskRadius" (int): the MfSegmentation tunables (MaskFusion.h:234-263 / MfSegmentation.h:42-62)
 *
 * Implementation switches (flags unless legal values are given; the defaults, in parentheses, are the product; the alternatives exist for A/B
 * measurements and as executable specifications):
 *   "splatTiles" (1)
 *   "globalTiles" (1: GlobalProjection of the background through tile lists)
 *   "gpuLabels" (1: label stage on the device)
 *   "batchTracking" (1: one Gauss-Newton launch serves every tracked model)
 *   "batchSolveInPixelPass" (1: an iteration of the batched Gauss-Newton loop is ONE launch -- every workgroup of a model finishes the previous
 *     iteration in its prologue, as the single-model kernel does; 0: a solve launch and a pixel launch per iteration; same bytes)
 *   "slabCulling" (1: the batched Gauss-Newton pixel pass skips the workgroups none of whose pixels can project onto a model's normals -- exact,
 *     mf_odometry.hip; 0: every workgroup walks its pixels)
 *   "earlyBackgroundFusion" (1)
 *   "cleanTap16" (1: inside mf_process_frame the index pass that feeds Model::clean writes one 16-byte tap per texel -- {x, y, z', initTime}, z' = NaN
 *     unless index > 0, confidence > the model's threshold and z > 0, its sign bit set when lastTime == tick: everything the pass's window uses of a
 *     tap, so the results are bit-identical -- and the filtered depth into a plane of its own; 0: the 32-byte record, which the model-level calls
 *     mf_model_predict_indices -> mf_model_clean always use)
 *   "cleanTapGroup" (3; legal: 1, 3, 9.  3: with 16-byte taps Model::clean requests the three taps of a window column together before it looks at
 *     the first; 1: one tap after the other; 9: the whole window at once -- the counts are integer sums, the results the same)
 *   "maskFreeClean" (1: in a context that takes no masks the background's clean pass and the index pass that feeds it carry no mask / depth plane
 *     -- no texel can disagree with model 0 --; 0: the planes travel in every context; a context with masks and the model-level calls always carry
 *     them)
 *   "fuseLanes" (4; legal: 1, 4.  4: the data association handles a candidate on a quad of lanes, one window column per lane, merged in the serial
 *     order; 1: one lane per candidate -- same results)
 *   "cleanLiteralWindow" (1: Model::clean walks its window with copy_unstable.vert's own fp32 trip count, 4 or 5 taps per axis; 0: 4 x 4)
 *   "objectSmallGrids" (1: the grid-stride surfel kernels of an object model run on a grid sized from its last known surfel count instead of 2048
 *     workgroups)
 *   "objectScatterSplat" (1: object models are predicted with the scatter form of the splat instead of tile lists) -- both leave every result
 *     bit-identical; measured on MI355X on the 12-model S2 scene: 394 -> 407 frames/s with both (profiles/r03a_bench_2s_object_switches.txt), on
 *     since round 3
 *   "batchObjectPasses" (1: the surfel passes of all object models of a frame as one launch per pass; 0: model by model, the executable
 *     specification)
 *   "objectStream" (1: inside mf_process_frame those batched launches -- the objects' fuse / clean chain and their prediction -- go to a second
 *     stream and run beside the background's chain, joined at the end of the frame; 0: one stream; same bytes)
 *   "cullRuns" (1; 0: big maps walk every run of the buffer in every projection pass and in Model::clean -- the executable specification of the
 *     culled forms)
 *   "literalFusionWeight" (1: Model::computeFusionWeight's log map takes cos(theta) from the float trace of a float matrix as the reference's text
 *     does -- its rotation term is then quantised in steps of ~4.9e-4 rad; 0: the same formula evaluated accurately in double.  See DESIGN.md,
 *     finding F5; default 1 since round 3)
 *   "frameToFrameRGB" (0; MaskFusion::setFrameToFrameRGB, "-ftf": the photometric term tracks against the previous RAW frame,
 *     Model.cpp:399-400,981)
 *   "objectBoundingBoxLimit" (1: Model::fuse limits an object model's depth by its bounding box + 5 % as upstream does whenever its GUI draws the
 *     models, Model.cpp:480-501; 0: bb_max_z = FLT_MAX, a headless upstream)
 *   "fusedRgbPyramid" (1: the frame's intensity pyramid and its derivative / gate images -- photometric term, SO(3) -- as one LDS-tiled launch;
 *     0: imageBGRToIntensity + 2 x pyrDownUcharGauss + computeDerivativeImages as four launches, the executable specification; same bytes)
 *   "fusedPreprocessLaunch" (1: when only the background is tracked model by model, its model-side pyramid is built in the depth filter's launch
 *     -- two independent kernels of a frame side by side; 0: two launches; same bytes)
 *   "deferPredict" (1; a single-model context that tracks with the geometric term alone, timings off: the prediction of frame t is enqueued at the
 *     head of the next mf_process_frame[_dev] call -- or by whatever other call on the context comes first -- instead of at the end of frame t, so
 *     that it can share launches with frame t + 1's preprocessing; same bytes.  Work the caller enqueues on mf_get_stream()'s stream sees frame t's
 *     prediction only behind the next library call)
 *   "fusedBinFilter" (1) / "fusedFramePyramids" (1) (in that head: the prediction's binning pass in the next frame's depth filter's launch / the
 *     frame's pyramid and the model-side pyramid in one launch; 0: two launches each; same bytes)
 *   "tilePyramid" (1: in that head every workgroup of the prediction's tile pass also writes its tile of the model-side pyramid, as the pyramid's
 *     own launch computes it without fill-in, and that launch becomes a fix-up whose workgroups leave at once unless the frame's fill-in decision
 *     is 1; 0: the model-side pyramid as a launch of its own; same bytes)
 *   "fusedTilePyramid" (needs "tilePyramid"; 1: the frame's pyramid rides in the tile pass's launch, in workgroups of its own; 0: it shares the
 *     fix-up's launch or, with "fusedFramePyramids" 0, runs alone; same bytes)
 *   "hostInputAsync" (1: mf_process_frame returns when the frame is enqueued; 0: the blocking form of rounds 1-3.  Setting it synchronises both
 *     streams first)
 *   "hostLockstep" (1: mf_process_frame waits for frame k-2 to have run before it enqueues frame k's upload)
 *   "hostWaitUpload" (1: ... and for its own upload: single-model frames)
 *   "modelApiPackedIndex" (0; 1: mf_model_predict_indices also builds the packed column-major map mf_process_frame feeds Model::clean with)
 *
 * Tuning knobs (int):
 *   "bigMapElements" (6 000 000: from this many surfels on a model's buffer is kept as RUNS with a table (Surfels::box): Model::clean works in
 *     place on the runs in which its rules can change something (k_cull_clean / k_clean_runs, the frame's new surfels appended behind the last
 *     run) and the projection passes visit only the runs that can be in view (k_cull) -- below, the two-launch clean (a dense copy) and
 *     whole-buffer passes of rounds 1-4)
 *   "inPlaceElements" (1 000 000: from this many surfels on update.vert runs in place -- below, as rounds 1-4's copy with the second index
 *     scatter riding on it); which form a model's passes take depends on its size alone and changes no result
 *     (tests/test_gpu_switches.py::test_clean_forms_agree)
 *   "tileHeight" (24; legal: 16, 20, 24, 32: tiles of 16 pixels by that many rows), "tileThreads" (512; legal: 256, 320, 384, 512, 1024: threads
 *     per tile workgroup), "spriteLanes" (4; legal: 1, 2, 4, 8, 16: lanes that share a sprite in the tile z-test): launch shape of the tile
 *     passes (A/B)
 *
 * Test knobs and actions:
 *   "densifyEvery" (int, 0; n > 0: a sparse buffer is compacted every n frames whatever the host's bounds say -- a test switch; by default only
 *     when the slots behind the last run or the table entries could run out, before a download, before a model returns to the small-map forms)
 *   "splatTileEntries" (int; legal: 1 up to its initial value.  Test knob: shrinks the tile lists to force their overflow path)
 *   "timings" (0; mf_get_timings), "passTimings" (0; mf_get_pass_timings; setting it clears the recorded passes), "icpProfile" (0)
 *   "splatProfile" (0; 1: per-tile stamps of the background's tile pass, debug tap "splat_prof"; MF_ENOMEM when its buffer cannot be allocated)
 *   "hostProfileReset" (write-only: restarts the host clocks below)
 *   "rebuildRunTable" (write-only: rebuilds the background's run table from scratch)
 *
 * Read-only taps (mf_get_param):
 *   "indexPackedTexelBytes" (16 or 32: the form the debug tap "index_packed" holds)
 *   "deferredFrames" / "fusedHeadFrames" (predictions deferred / frames that took the fused head so far)
 *   "pyramidFixupFrames" (fused heads whose fix-up rebuilt the pyramid, i.e. whose tracking step fills in; synchronises the stream)
 *   "densifyCount" (compactions so far)
 *   "cleanRuns" / "visibleRuns" / "backgroundRuns" (runs the last in-place clean visited / runs k_cull listed for the last pass / runs of the
 *     background's table)
 *   "unstampedRuns" (live runs of that table that hold a surfel with lastTime <= 0: the in-place clean visits them every frame)
 *   "hostStageUs" | "hostUploadUs" | "hostEnqueueUs" | "hostCallUs" | "hostWaitUs" (host clocks inside mf_process_frame, microseconds per call
 *     since mf_set_param("hostProfileReset", 1)) */
int mf_set_param(mf_ctx* ctx, const char* key, double value);
int mf_get_param(mf_ctx* ctx, const char* key, double* value);

/* Stage timings in the reference's Stopwatch label set (Core/Utils/Stopwatch.h:46-121): GPU milliseconds of the
 * last frame measured with HIP events when enabled by mf_set_param("timings", 1).
 * labels: 0 Preprocess, 1 odomInit (model-side pyramids of the background model), 2 odom (all tracking), 3 indexMap,
 *         4 Fuse::Data, 5 Fuse::Update, 6 Fuse::Copy, 7 IndexMap::ACTIVE, 8 Run,
 *         9 icpIterations: first to last Gauss-Newton iteration launch of the background model (what bench.py divides by
 *           the iteration count for its roofline line);
 *         10 icpCoarse / 11 icpFine: the same interval split right before the first level-0 iteration (launch-per-iteration loop of a
 *           single model; 0 for the batched form);
 *         multi-model frames only (0 otherwise) -- what lies between the end of tracking and Fuse::Copy's end (labels 3..6 cover the
 *         BACKGROUND's passes there; Core/MaskFusion.cpp:287-375,539-565):
 *         12 mmGlobalProjection (GlobalProjection::project of every model + id resolve), 13 mmEdgeLabels (geometric edge map, binary
 *         edges, the device label stage), 14 mmBackgroundFuseClean (the background's predictIndices / fuse / clean, enqueued ahead of
 *         the host's look at the label stage's decision), 15 mmHostStall (GPU idle between the end of that and the first object pass:
 *         the host had not enqueued it yet), 16 mmObjectFuseClean (spawn pass + every object model's predictIndices / fuse / clean),
 *         17 mmHostWaitMs (HOST wall-clock milliseconds spent in the event wait behind the label stage) */
#define MF_N_TIMINGS 18
int mf_get_timings(mf_ctx* ctx, float* ms /* [MF_N_TIMINGS] */);
/* The surfel passes of the last frame one by one (Core/Model/Model.cpp:466-772, ModelProjection.cpp:100-268, GlobalProjection.cpp:43-107): GPU
 * milliseconds between two HIP events recorded around each pass's launches, enabled by mf_set_param("passTimings", 1).  `bg`: the background
 * model (or any model handled on its own); `obj`: every object model, one launch per pass for all of them.
 *   0 bgGlobalProjection   k_cull + k_splat_bin + k_global_tile
 *   1 bgIndexMap           k_cull (if not shared) + k_index_scatter + resolve: predictIndices before fuse
 *   2 bgFuseData           k_fuse_data: association
 *   3 bgFuseUpdate         k_fuse_update[_copy]: update.vert
 *   4 bgIndexMap2          k_index_scatter + packed resolve: predictIndices after fuse (rides on the copy-update of small maps)
 *   5 bgClean              Model::clean of the buffer's own surfels: k_cull_clean + k_clean_runs (in place) / the two-launch form (everything)
 *   6 bgAppend             ... and of the frame's candidates, appended (in-place form only)
 *   7 bgPredict            combinedPredict: k_cull + k_splat_bin + k_splat_tile (+ the end-of-frame bookkeeping)
 *   8 objGlobalProjection  9 objFuseClean (predictIndices, fuse, predictIndices, clean)   10 objPredict
 *   11 compaction          launch_densify + the run table of the compacted buffer (0 in a frame without one)
 * With "objectStream" on, rows 9 and 10 are timed on the object stream, where they run BESIDE rows 1-7: each row is then longer than the pass on
 * its own and the rows no longer add up to the frame.  For passes on their own, switch the stage timings on as well ("timings": they keep the frame
 * on one stream) or set "objectStream" to 0 -- bench.py's roofline_passes does the former. */
#define MF_N_PASSES 12
enum { MF_PASS_BG_GLOBAL = 0, MF_PASS_BG_INDEX, MF_PASS_BG_FUSE_DATA, MF_PASS_BG_FUSE_UPDATE, MF_PASS_BG_INDEX2, MF_PASS_BG_CLEAN, MF_PASS_BG_APPEND,
       MF_PASS_BG_PREDICT, MF_PASS_OBJ_GLOBAL, MF_PASS_OBJ_FUSE_CLEAN, MF_PASS_OBJ_PREDICT, MF_PASS_COMPACTION };
int mf_get_pass_timings(mf_ctx* ctx, float* ms /* [MF_N_PASSES] */);
/* The context's HIP stream (hipStream_t), for callers that time with their own events. */
void* mf_get_stream(mf_ctx* ctx);
/* Stream on which rgb/depth/mask handed to mf_process_frame_dev are first read: the context's stream (mf_get_stream) -- producers ordered on
 * it need no further synchronisation; a buffer stays unmodified until its frame has completed there.  (Rounds 2-4 could move the
 * pose-independent preprocessing to a second stream, "overlapPreprocessing"; it never gained anything -- also not with that stream masked to
 * a few compute units, round 5 -- and is gone.  The entry point stays so that callers written against it keep working.) */
void* mf_get_input_stream(mf_ctx* ctx);

/* debug / differential-test taps: copy a device-resident intermediate of the last frame to host.
 * what: "depthF" (H*W f32), "vmap0".."vmap2", "nmap0".."nmap2" (3*h*w f32, current frame),
 *       "vmap_g0".."vmap_g2", "nmap_g0".."nmap_g2" (model side), "pred_vertex", "pred_normal" (H*W*4 f32),
 *       "pred_image" (H*W*4 u8), "pred_time" (H*W u16), "icp_log" (19*32 f32: per-iteration A-upper/b/res/inl),
 *       "gn_trace" (20*64 f64, geometric loop: row r = the reduced system of iteration r as summed in fp64 [0..31], then resultRt [32..47],
 *       Rcurr [48..56], tcurr [57..59] as iteration r used them; row 19 = the state after the last update),
 *       "edge_map" (H*W f32), "edge_binary" (H*W u8), "projected_ids" (H*W u8);
 *       index map of the last (pre-fusion) index pass, index_map.frag's attachments: "index" (H*W i32), "index_vc", "index_nr",
 *       "index_ct" (H*W*4 f32), "index_packed" (post-fusion pass, column-major texel order: 2 float4 per texel, or -- when the last frame ran
 *       with "cleanTap16" -- 1 float4 per texel {x, y, z', initTime}; "indexPackedTexelBytes" tells which);
 *       Model::fuse / clean intermediates (variable length: as many bytes as asked for, at most the buffer): "cand_op" (u8 per
 *       quarter-rate pixel in column-major order: 0 none, 1 merge, 2 new), "cand_rec" (3 float4 per candidate), "clean_flags"
 *       (u8 keep flag per old surfel, then per candidate), "clean_newconf" (f32, same indexing). */
int mf_debug_read(mf_ctx* ctx, const char* what, void* out, uint64_t out_bytes);

/* ------------------------------------------------------------------------------------------------
 * Model-level entry points: the public operations of Model (Core/Model/Model.h:126-162,233-268), one call each, on a
 * frame staged with mf_stage_frame.  MaskFusion::processFrame is a fixed composition of them (mf_process_frame enqueues the
 * same kernels); they let a caller drive a model the way the reference's callers do, and let every surfel pass be compared
 * with the oracle in isolation.  `model` is the index in the model list (as in mf_get_pose).  All calls are asynchronous on
 * the context's stream except where noted.  The index map, the association candidates and the new-surfel records are
 * scratch shared by all models: predictIndices -> fuse -> [predictIndices] -> clean of ONE model must not be interleaved
 * with another model's (the reference keeps those buffers per model, ModelProjection / Model::newUnstableBuffer).
 * ---------------------------------------------------------------------------------------------- */
/* Everything of processFrame that touches no model: upload, MaskFusion::filterDepth (Core/MaskFusion.cpp:217,650-657),
 * Model::generateCUDATextures (Core/Model/Model.h:128, Model.cpp:350-389), the intensity pyramid / derivative images
 * (RGBDOdometry::initRGB).  mask = model id per pixel as textureMask holds it for fuse / clean (Core/MaskFusion.cpp:297);
 * NULL = leave textureMask as it is (all background in a fresh context).  Host pointers; synchronous. */
int mf_stage_frame(mf_ctx* ctx, const uint8_t* rgb, const float* depth, const uint8_t* mask);
/* The same for a frame that is already in device memory (no upstream twin: upstream's FrameData lives on the host, MaskFusion.cpp:212-216
 * uploads it).  Asynchronous: producers of the buffers are ordered on mf_get_stream(ctx) by the caller (e.g. an RCCL broadcast enqueued
 * there), and d_rgb / d_depth stay valid and unmodified until the model-level calls of this frame have completed on that stream. */
int mf_stage_frame_dev(mf_ctx* ctx, const uint8_t* d_rgb, const float* d_depth, const uint8_t* d_mask);
/* The tail of processFrame (Core/MaskFusion.cpp:569-602) for a frame driven through the calls below: tick++, the
 * requiresFillIn decision for the next tracking step, the pose-log entry with `timestamp`, age++ */
int mf_end_frame(mf_ctx* ctx, int64_t timestamp);
/* The three per-model LOOPS of MaskFusion::processFrame over this context's model list, for a caller that sequences a frame itself
 * (one scene sharded by model over several contexts).  They run what mf_process_frame runs for these loops -- ONE batched
 * Gauss-Newton loop over all tracked models, ONE launch per surfel pass for all object models -- under the context's configuration.
 * first_model = 0: the whole list; 1: models[0] is the stand-in of a background owned by another context (pose via
 * mf_model_override_pose; neither tracked, fused nor drawn, but its tick advances).
 *   mf_track_models    Core/MaskFusion.cpp:247-276 (trackableClassIds, updateStaticPose for static objects, the 0.2 m jump rule)
 *   mf_fuse_models     :335-339, :369-374 (setMaxDepth, confidence ramp), :342-353 for models[spawned_model] when spawned_model >= 1
 *                      (-1: none), then the fusion loop :539-565
 *   mf_predict_models  :569 predict(), :573 tick++, :580-596 pose log, :600 incrementAge -- the end of such a frame (instead of
 *                      mf_model_combined_predict per model + mf_end_frame) */
int mf_track_models(mf_ctx* ctx, int32_t first_model, int32_t track_all_models);
int mf_fuse_models(mf_ctx* ctx, int32_t first_model, float weight_multiplier, int32_t spawned_model);
int mf_predict_models(mf_ctx* ctx, int32_t first_model, int64_t timestamp);
/* Model::initialise (Core/Model/Model.h:126, Model.cpp:240-285) from the staged frame */
int mf_model_initialise(mf_ctx* ctx, int32_t model);
/* Model::overridePose (Core/Model/Model.h:235-238): lastPose = pose; pose = pose16 */
int mf_model_override_pose(mf_ctx* ctx, int32_t model, const float* pose16);
/* Model::computeFusionWeight(weightMultiplier) (Core/Model/Model.cpp:449-464) of the model's pose / lastPose.  Synchronous. */
int mf_model_fusion_weight(mf_ctx* ctx, int32_t model, float weight_multiplier, float* out);
/* Model::performTracking (Core/Model/Model.h:135-136, Model.cpp:427-447); the rgb texture is the staged frame's.  frame_to_frame_rgb
 * ("-ftf", GUI/MainController.cpp:252,539): initRGBModel takes the fill-in image -- the previous RAW frame when the last prediction ran
 * with mf_set_param("frameToFrameRGB", 1) (Model.cpp:981) -- instead of the model's RGB projection (Model.cpp:399-400); models that
 * allow no fill-in (objects) are unaffected, as upstream.  MF_ESTATE when a photometric term is requested on a context that built no
 * intensity / derivative images (icpWeight >= 100 and no rgbOnly). */
int mf_model_perform_tracking(mf_ctx* ctx, int32_t model, int32_t frame_to_frame_rgb, int32_t rgb_only, float icp_weight,
                              int32_t pyramid, int32_t fast_odom, int32_t so3, float max_depth_processed, int64_t log_timestamp,
                              int32_t try_fill_in);
/* Model::predictIndices(time, maxDepth, timeDelta) (Core/Model/Model.h:162, ModelProjection.cpp:100-152) */
int mf_model_predict_indices(mf_ctx* ctx, int32_t model, int32_t time, float max_depth, int32_t time_delta);
/* Model::fuse(time, rgb, mask, depthRaw, depthFiltered, depthCutoff, weightMultiplier) (Core/Model/Model.h:142-143,
 * Model.cpp:466-647); the four textures are the staged frame's */
int mf_model_fuse(mf_ctx* ctx, int32_t model, int32_t time, float depth_cutoff, float weight_multiplier);
/* Model::clean(time, graph, timeDelta, depthCutoff, isFern, depthFiltered, mask) (Core/Model/Model.h:146-147,
 * Model.cpp:649-772); no deformation graph, isFern = false (loop closure is dead code upstream) */
int mf_model_clean(mf_ctx* ctx, int32_t model, int32_t time, int32_t time_delta, float depth_cutoff);
/* Model::combinedPredict(maxDepth, time, maxTime, timeDelta, ACTIVE) (Core/Model/Model.h:158, ModelProjection.cpp:187-268);
 * time must equal max_time (the only form the reference calls, Core/MaskFusion.cpp:616-628) */
int mf_model_combined_predict(mf_ctx* ctx, int32_t model, float max_depth, int32_t time, int32_t max_time, int32_t time_delta);
/* No upstream twin (tests, tooling): replace the surfel buffer of `model` with `count` records in mf_download_map's layout.
 * Host pointer; synchronous. */
int mf_model_upload_map(mf_ctx* ctx, int32_t model, const float* surfels12, uint32_t count);
/* Model::makeNonStatic / makeStatic(globalPose) (Core/Model/Model.h:263-266): a non-static object model is tracked even with
 * trackAllModels off (Core/MaskFusion.cpp:263); makeStatic re-anchors it to the background's current pose */
int mf_make_nonstatic(mf_ctx* ctx, int32_t model);
int mf_make_static(mf_ctx* ctx, int32_t model);
/* MaskFusion::setTrackableClassIds (Core/MaskFusion.h:246, MaskFusion.cpp:261,940); n = 0: every class is trackable */
int mf_set_trackable_class_ids(mf_ctx* ctx, const int32_t* ids, int32_t n);
/* mf_debug_read for the per-model taps ("pred_vertex", "pred_normal", "pred_image", "pred_time") of model `model` */
int mf_debug_read_model(mf_ctx* ctx, int32_t model, const char* what, void* out, uint64_t out_bytes);

/* ------------------------------------------------------------------------------------------------
 * Model-sharded scenes: several contexts -- one per GPU -- each own some of the models of ONE scene.  What
 * MaskFusion::processFrame couples between models crosses the contexts through these calls: the z-merged model-id image
 * (GlobalProjection, Core/Model/GlobalProjection.cpp:43-114), the label image (Core/MaskFusion.cpp:289-297) and the background
 * pose (static objects follow it, Core/Model/Model.h:263-264; mf_model_override_pose(ctx, 0, pose) installs it on a context
 * that does not own the background).  maskfusion_amd/sharded.py sequences them with the Model-level calls above and with
 * collectives (all-reduce(MIN) of the keys, broadcast of labels + pose + control record, gather of per-model state).
 * ---------------------------------------------------------------------------------------------- */
/* GlobalProjection::project of this context's models only.  d_keys_out: width*height uint64 = float_bits(z) << 32 | order << 8 | id,
 * all ones = empty; the per-pixel minimum over contexts is the merged image.  orders[i]: position of local model i in the GLOBAL
 * model list (the GL draw order that breaks exact depth ties), < 0: do not draw it (a background stand-in). */
int mf_export_projection_keys_dev(mf_ctx* ctx, const int32_t* orders, int32_t n_orders, uint64_t* d_keys_out);
/* GlobalProjection::downloadDirect of a merged key image: sets the projected-id image of the next mf_perform_segmentation */
int mf_import_projection_keys_dev(mf_ctx* ctx, const uint64_t* d_keys);
/* MaskFusion::performSegmentation (Core/MaskFusion.h:59; MfSegmentation.cpp:83-538) on the staged frame.  mask: host, H*W mask ids
 * or NULL.  model_ids NULL: this context's model list; else the GLOBAL list in order (index 0 = background) with next_model_id
 * = MaskFusion::getNextModelID().  Result -> textureMask; *has_new_label / *new_class_id = SegmentationResult::hasNewLabel and
 * the class of the new label.  Synchronous. */
int mf_perform_segmentation(mf_ctx* ctx, const uint8_t* mask, const int32_t* class_ids, int32_t n_masks, const int32_t* model_ids,
                            const int32_t* model_class_ids, int32_t n_models, int32_t next_model_id, int32_t allow_new,
                            int32_t* has_new_label, int32_t* new_class_id);
/* The same in two halves (what mf_process_frame does with "earlyBackgroundFusion"): _begin enqueues the label stage and returns; the caller
 * may then enqueue work that does not depend on the decision -- mf_fuse_background: the background is never spawned or dropped and its
 * fusion (Core/MaskFusion.cpp:539-565 for models.front()) reads only the label image, complete on the stream -- and _end waits for the
 * label stage alone.  mf_fuse_models skips a background that mf_fuse_background has already fused for the staged frame. */
int mf_perform_segmentation_begin(mf_ctx* ctx, const uint8_t* mask, const int32_t* class_ids, int32_t n_masks, const int32_t* model_ids,
                                  const int32_t* model_class_ids, int32_t n_models, int32_t next_model_id, int32_t allow_new);
int mf_perform_segmentation_end(mf_ctx* ctx, int32_t* has_new_label, int32_t* new_class_id);
int mf_fuse_background(mf_ctx* ctx, float weight_multiplier);
/* SegmentationResult::fullSegmentation as device memory: out of the context that ran the label stage, into the others
 * (textureMask->Upload, Core/MaskFusion.cpp:297) */
int mf_export_segmentation_dev(mf_ctx* ctx, uint8_t* d_out);
int mf_import_segmentation_dev(mf_ctx* ctx, const uint8_t* d_in);
/* MaskFusion::spawnObjectModel (Core/MaskFusion.cpp:671-684) with the id the label-stage owner allocated */
int mf_spawn_object_model(mf_ctx* ctx, int32_t id, int32_t class_id);
/* MaskFusion::inactivateModel (Core/MaskFusion.cpp:686-713) */
int mf_drop_model(mf_ctx* ctx, int32_t model);
/* Inactive models (MaskFusion::inactiveModels, MaskFusion.h:398; DESIGN.md "Inactive models and re-detection").  With
 * mf_set_param("keepInactiveModels", 1) a model that mf_drop_model or the jump rule of mf_process_frame retires is first ARCHIVED when line 702
 * keeps it (the rule: the parameter list above): its map's records exactly as mf_download_map would return them at that moment -- compacted,
 * in the live order, also for a map kept as runs -- in a device buffer of exactly that size, and the info below.  Keeping synchronises the
 * context's streams and allocates; with the key at 0 (the default) nothing of this happens and a drop is what it was.  The list is in the
 * order of the drops; k indexes it, and every call returns MF_EINVAL for a k outside it.  Upstream declares the way back
 * (MaskFusion::redetectModels, Model::detectInRegion) and ships it empty; here recognition is maskfusion_amd.redetect, driven from Python. */
typedef struct mf_inactive_info_t {
    int32_t id, class_id;           /* Model::getID(), getClassID() */
    uint32_t surfels;               /* records in the archive */
    uint32_t age;                   /* Model::age at the drop */
    float confidence_threshold;     /* Model::getConfidenceThreshold() at the drop */
    int32_t tick;                   /* mf_get_tick at the drop */
    float pose[16];                 /* the model's last pose, column-major as mf_get_pose */
} mf_inactive_info_t;
int mf_inactive_count(mf_ctx* ctx, int32_t* n);
int mf_inactive_info(mf_ctx* ctx, int32_t k, mf_inactive_info_t* out);
/* the archive in DEVICE memory: *n records of 12 floats (NULL for an empty map); valid until the list changes (a kept drop, a discard, a
 * reactivation, mf_destroy) */
int mf_inactive_map_dev(mf_ctx* ctx, int32_t k, const float** d_records, uint32_t* n);
/* as mf_download_map: min(*count, max_count) records into host memory */
int mf_inactive_download_map(mf_ctx* ctx, int32_t k, float* out, uint32_t max_count, uint32_t* count);
/* frees entry k; the later entries move up */
int mf_inactive_discard(mf_ctx* ctx, int32_t k);
/* No upstream twin: sets an object model's age and confidence threshold (what processFrame's ramp, Core/MaskFusion.cpp:369-374, derives from
 * the age every frame).  MF_EINVAL for the background or a threshold that is negative or NaN. */
int mf_model_set_age(mf_ctx* ctx, int32_t model, uint32_t age, float confidence_threshold);
/* Brings entry k back into the model list.  DEFINED as this sequence of public calls, whose bits it leaves:
 *   1. mf_spawn_object_model(archived id, archived class) -- MF_EINVAL, "model id in use", when a live model has the id; the entry then stays;
 *   2. mf_model_upload_map of the archive;
 *   3. mf_model_override_pose(pose16, or the archived pose when pose16 is NULL; column-major);
 *   4. mf_make_nonstatic;
 *   5. mf_model_set_age(archived age, archived confidence threshold).
 * The entry then leaves the list and the later entries move up.  The model's pose log starts anew; mf_export_poses writes the retired
 * segment(s) of an id and then the live one into the one poses-<id>.txt, which is time order. */
int mf_reactivate_model(mf_ctx* ctx, int32_t k, const float* pose16);
/* Merges `count` records (HOST, mf_download_map's layout) into the live map of `model`.  DEFINED as this sequence of public calls, whose bits
 * it leaves:
 *   1. mf_download_map of the model: the targets;
 *   2. mf_cloud_merge_dev(targets, source12, source_to_model16 (HOST, column-major, or NULL), radius, min_cos) on mf_get_stream(ctx), into a
 *      buffer of n_target + count records;
 *   3. mf_model_upload_map of the merged records.
 * The model keeps its pose, age, id, class and static flag.  stats4 as mf_cloud_merge_dev's (may be NULL).  A merged map larger than the
 * model's surfel buffer fails as mf_model_upload_map fails (MF_EINVAL) and leaves the model as it was; stats4 is filled all the same.  The map
 * makes a round trip through host memory: a tool's call, not a frame's. */
int mf_model_merge_map(mf_ctx* ctx, int32_t model, const float* source12, uint32_t count, const float* source_to_model16, float radius,
                       float min_cos, uint64_t stats4[4]);
/* Model::updateStaticPose(globalPose) (Core/Model/Model.h:263) with this context's background pose */
int mf_model_update_static_pose(mf_ctx* ctx, int32_t model);
/* Model::setMaxDepth + the object confidence ramp of processFrame (Core/MaskFusion.cpp:335-339,369-374) for the local objects */
int mf_update_object_params(mf_ctx* ctx);

/* ------------------------------------------------------------------------------------------------
 * Kernel-level entry points (device pointers, launched on `stream`, asynchronous).  Each replaces one reference
 * CUDA wrapper or GLSL pass; the parity tests call them one by one against oracle/.
 * ---------------------------------------------------------------------------------------------- */
/* MaskFusion::filterDepth + depth_bilateral_metric.frag (Core/MaskFusion.cpp:650-657) */
int mf_k_bilateral(const float* d_depth, float* d_out, int32_t W, int32_t H, void* stream);
/* pyrDownGaussF (Core/Cuda/cudafuncs.cu:510-532) */
int mf_k_pyrdown_f(const float* d_src, float* d_dst, int32_t sw, int32_t sh, void* stream);
/* createVMap + createNMap (Core/Cuda/cudafuncs.cu:136-150,191-205), one level; planar [3][H][W] outputs */
int mf_k_vmap_nmap(const float* d_depth, float* d_vmap, float* d_nmap, int32_t W, int32_t H, float fx, float fy,
                   float cx, float cy, float depth_cutoff, void* stream);
/* RGBDOdometry::initICPModel (Core/Utils/RGBDOdometry.cpp:153-185): copyMaps + resizeVMap/NMap x2 + tranformMaps x3.
 * d_v4/d_n4: H*W float4 predictions; outputs: 3 levels planar, packed level after level; R row-major 3x3 */
int mf_k_model_pyramid(const float* d_v4, const float* d_n4, const float* R9, const float* t3, float* d_vmaps,
                       float* d_nmaps, int32_t W, int32_t H, void* stream);
/* computeGeometricSegmentationMap -> thresholdMap -> morphGeometricSegmentationMap -> invertMap
 * (Core/Cuda/segmentation.cu:277-354; MfSegmentation.cpp:149-207).  d_vmap/d_nmap: level-0 planar maps;
 * d_edge: H*W f32 out; d_binary: H*W u8 out (255 = not an edge); d_tmp: H*W u8 scratch */
int mf_k_geometric_edges(const float* d_vmap, const float* d_nmap, float* d_edge, uint8_t* d_binary, uint8_t* d_tmp,
                         int32_t W, int32_t H, float w_distance, float w_convexity, float threshold, int32_t morph_radius,
                         int32_t morph_iterations, void* stream);
/* Host half of MfSegmentation::performSegmentation (Core/Segmentation/MfSegmentation.cpp:220-522): HOST pointers, no GPU
 * involved (the reference runs this stage on the CPU too).  binary: 255 = not an edge; params: {threshold, weightDistance,
 * weightConvexity, morphEdgeIterations, morphEdgeRadius, morphMaskIterations, morphMaskRadius, removeEdges,
 * minRelSizeNew, maxRelSizeNew, personClassID} (MfSegmentation.h:42-62); ignore_map: persistent H*W in/out. */
int mf_segmentation_labels(int32_t W, int32_t H, const uint8_t* binary, const float* depth, const uint8_t* mask,
                           const int32_t* class_ids, int32_t n_masks, const uint8_t* projected_ids, const int32_t* model_ids,
                           const int32_t* model_class_ids, int32_t n_models, int32_t next_model_id, int32_t allow_new,
                           const float* params11, uint8_t* ignore_map, uint8_t* full_segmentation, int32_t* has_new_label,
                           int32_t* new_class_id);
/* The same stage on the device (what mf_process_frame uses unless mf_set_param("gpuLabels", 0)): identical
 * arguments and results, HOST pointers (staged internally). */
int mf_k_segmentation_labels(int32_t W, int32_t H, const uint8_t* binary, const float* depth, const uint8_t* mask,
                           const int32_t* class_ids, int32_t n_masks, const uint8_t* projected_ids, const int32_t* model_ids,
                           const int32_t* model_class_ids, int32_t n_models, int32_t next_model_id, int32_t allow_new,
                           const float* params11, uint8_t* ignore_map, uint8_t* full_segmentation, int32_t* has_new_label,
                           int32_t* new_class_id);
/* The device stage with its intermediates readable (what mf_k_segmentation_labels calls with the extra arguments null).
 * alive: nullable, one flag per model, 0 = dropped by the 0.2 m jump rule in this frame (entry 0, the background, is ignored).
 * Outputs, each nullable, HOST pointers: lab_cc [W*H] component labels in cv::connectedComponentsWithStats numbering; lab_swept
 * [W*H] the labels the votes read (after the removeEdges sweeps); stats5 [min(n_comp, stats_cap) x 5] left, top, width, height,
 * area per component (row 0, the background, is not written); n_comp: components including the background.  They are written
 * even where the call returns MF_ESTATE because the vote tables would not fit. */
int mf_k_label_stage(int32_t W, int32_t H, const uint8_t* binary, const float* depth, const uint8_t* mask,
                     const int32_t* class_ids, int32_t n_masks, const uint8_t* projected_ids, const int32_t* model_ids,
                     const int32_t* model_class_ids, int32_t n_models, int32_t next_model_id, int32_t allow_new,
                     const float* params11, uint8_t* ignore_map, uint8_t* full_segmentation, int32_t* has_new_label,
                     int32_t* new_class_id, const int32_t* alive, int32_t* lab_cc, int32_t* lab_swept, int32_t* stats5,
                     int32_t* n_comp, int32_t stats_cap);
/* imageBGRToIntensity (Core/Cuda/cudafuncs.cu:626-654); channels = 3 or 4, the first three are used as stored */
int mf_k_intensity(const uint8_t* d_img, int32_t channels, uint8_t* d_out, int32_t n, void* stream);
/* pyrDownUcharGauss (Core/Cuda/cudafuncs.cu:534-588) */
int mf_k_pyrdown_u8(const uint8_t* d_src, uint8_t* d_dst, int32_t sw, int32_t sh, void* stream);
/* computeDerivativeImages (Core/Cuda/cudafuncs.cu:658-718) */
int mf_k_derivative_images(const uint8_t* d_src, int16_t* d_dx, int16_t* d_dy, int32_t W, int32_t H, void* stream);
/* The SO(3) block of RGBDOdometry::getIncrementalTransformation (Core/Utils/RGBDOdometry.cpp:264-324) with so3Step
 * (Core/Cuda/reduce.cu:999-1202) inside: level-2 images and intrinsics in, resultR (row-major double, host) and
 * {lastSO3Error, lastSO3Count, iterations} out.  Synchronous. */
int mf_k_so3_prealign(const uint8_t* d_last, const uint8_t* d_next, int32_t W, int32_t H, float fx, float fy, float cx,
                      float cy, double* R9, float* stats3, void* stream);
/* computeRgbResidual (Core/Cuda/reduce.cu:774-997).  d_corres: W*H records {int16 u0, int16 v0, float diff}
 * (u0 < 0: none) = DataTerm without the redundant fields; count_sigma2 (host) = {count, sum diff^2 as int32}.
 * Synchronous. */
int mf_k_rgb_residual(float min_scale, const int16_t* d_dIdx, const int16_t* d_dIdy, const float* d_last_depth,
                      const float* d_next_depth, const uint8_t* d_last_image, const uint8_t* d_next_image,
                      float max_depth_delta, const float* kt3, const float* krkinv9, int32_t W, int32_t H, void* d_corres,
                      int32_t* count_sigma2, void* stream);
/* mf_k_rgb_residual (which is this call with a null gate) with an optional gate image, W*H bytes as mf_k_rgb_gate returns
 * them: given, the border / 4x4 window / gradient tests are read from it, as a frame's iterations do, and min_scale, d_dIdx,
 * d_dIdy are not consulted.  Synchronous. */
int mf_k_rgb_residual_gated(float min_scale, const int16_t* d_dIdx, const int16_t* d_dIdy, const float* d_last_depth,
                            const float* d_next_depth, const uint8_t* d_last_image, const uint8_t* d_next_image,
                            float max_depth_delta, const float* kt3, const float* krkinv9, int32_t W, int32_t H,
                            void* d_corres, int32_t* count_sigma2, const uint8_t* d_gate_or_null, void* stream);
/* rgbStep (Core/Cuda/reduce.cu:529-713) with projectToPointCloud (Core/Cuda/cudafuncs.cu:722-751) evaluated on the
 * fly from d_last_depth; out32 (host, double) = {27 upper-tri products, row6^2, inliers, pad}.  Synchronous. */
int mf_k_rgb_step(const void* d_corres, float sigma, const float* d_last_depth, float fx, float fy, float cx, float cy,
                  const int16_t* d_dIdx, const int16_t* d_dIdy, float sobel_scale, int32_t W, int32_t H, double* out32,
                  void* stream);
/* One Gauss-Newton update exactly as the iteration kernels run it: the host side of getIncrementalTransformation
 * (Core/Utils/RGBDOdometry.cpp:428-474: Eigen LDLT solve of the 6x6 system in double, OdometryProvider::computeUpdateSE3 /
 * rodrigues, Core/Utils/OdometryProvider.h:32-90, currentT = [Rprev|tprev] * transform^-1) moved to the device.  HOST pointers.
 * sys29: the 27 upper-triangle products of the 7-vector row in reduce.cu:378-411 order, then sum r^2, then the inlier count;
 * result_rt16: resultRt before the step (row-major 4x4 double); Rprev9 / tprev3: the model pose the frame is tracked against.
 * Out: x6_serial (the production one-thread LDL^T), x6_wave (the wave-parallel Gauss-Jordan the RGB-D kernels use), the updated
 * resultRt, Rcurr / tcurr, stats2 = {lastICPError = sqrt(sum r^2) / inliers, lastICPCount}.  Synchronous. */
int mf_k_gn_solve(const double* sys29, const double* result_rt16, const float* Rprev9, const float* tprev3, double* x6_serial,
                  double* x6_wave, double* result_rt16_out, float* Rcurr9, float* tcurr3, float* stats2, void* stream);
/* icpStep (Core/Cuda/reduce.cu:446-525): d_out32 receives {27 upper-tri products, sum r^2, inliers, pad} */
int mf_k_icp_step(const float* Rcurr9, const float* tcurr3, const float* d_vmap_curr, const float* d_nmap_curr,
                  const float* Rprev_inv9, const float* tprev3, float fx, float fy, float cx, float cy,
                  const float* d_vmap_g_prev, const float* d_nmap_g_prev, float dist_thresh, float angle_thresh,
                  int32_t W, int32_t H, float* d_out32, void* stream);
/* mf_k_icp_step (form 0: k_icp_iter) through the other kernels that share its per-pixel functions, for the tests of the
 * correspondence gates: form 1 the batched pixel pass for one model, unfused, without slab culling; form 2 the same with slab
 * culling against rect4 = {x0, y0, x1, y1}, the level-0 rectangle of the model's normals (required); form 3 the RGB-D iteration
 * kernel with the geometric term on and a blank photometric level.  The same 32 floats.  Both entries return MF_EINVAL for a
 * threshold that is negative, NaN or infinite, before anything is allocated or launched.  Synchronous. */
int mf_k_icp_step_form(int32_t form, const float* Rcurr9, const float* tcurr3, const float* d_vmap_curr,
                       const float* d_nmap_curr, const float* Rprev_inv9, const float* tprev3, float fx, float fy, float cx,
                       float cy, const float* d_vmap_g_prev, const float* d_nmap_g_prev, float dist_thresh,
                       float angle_thresh, int32_t W, int32_t H, float* d_out32, const int32_t* rect4_or_null, void* stream);
/* The level-0 gate image (1 where the border, 4x4 window and gradient tests of RGBResidual::getProducts pass) from both kernels
 * that write it: d_gate_single, d_dIdx, d_dIdy from the derivative kernel on d_src; d_gate_pyramid from the one-launch pyramid
 * on an RGB image whose three channels equal d_src, with d_gray_pyramid, the intensity image that launch derived (the caller
 * checks that it equals d_src).  min_scale3: the three levels' thresholds (host).  *pyramid_ran = 0, and the two pyramid
 * outputs untouched, where W or H is no multiple of 4 (sizes the pyramid's tiling does not cover).  W, H >= 4.  Synchronous. */
int mf_k_rgb_gate(const uint8_t* d_src, int32_t W, int32_t H, const float* min_scale3, uint8_t* d_gate_single,
                  uint8_t* d_gate_pyramid, int16_t* d_dIdx, int16_t* d_dIdy, uint8_t* d_gray_pyramid, int32_t* pyramid_ran,
                  void* stream);
/* The launch form the geometric Gauss-Newton kernel takes for a pyramid level of W x H pixels (host only, no GPU involved):
 * out = {threads per workgroup, pixel slots per thread, workgroups, pixels per workgroup, workgroups that hold at least one
 * pixel}.  Read from the functions the launch itself calls, so that a test can name the form its image sizes select. */
int mf_k_icp_launch_form(int32_t W, int32_t H, int32_t out[5]);

/* ------------------------------------------------------------------------------------------------
 * Sessions: a running context saved to a file and resumed bit for bit (no upstream twin; DESIGN.md "Sessions").
 * A run that is saved, destroyed, loaded and continued leaves the same bits as a run that never stopped.
 * A session is read by the build of the library that wrote it: the file records sizeof(PoseDev), sizeof(FrameDev), sizeof(mf_config)
 * and the run length of the surfel tables, and a build in which one of them differs refuses the file.  Nothing more is promised across
 * versions of the library.
 *
 * THE FILE (little-endian; every offset from the start of the file):
 *   header, 64 bytes
 *      0  char[8]   magic "MFSESSN1"
 *      8  uint32    format version (MF_SESSION_VERSION)
 *     12  uint32    sizeof(PoseDev)      16  uint32  sizeof(FrameDev)      20  uint32  run length of the surfel tables (kRun)
 *     24  int32     image width          28  int32   image height
 *     32  int32     models in the list (the background included)
 *     36  int32     tick (mf_get_tick)
 *     40  uint64    bytes of the user blob
 *     48  uint32    sections             52  uint32  sizeof(mf_config)
 *     56  int64     frames the context has processed or staged
 *   section table at offset 64, 64 bytes per section
 *      0  char[32]  name, NUL-padded     32  int32   owner: index in the model list, or -1 (the context)
 *     36  uint32    0                    40  uint64  offset of the payload (a multiple of 256, behind the table)
 *     48  uint64    bytes of the payload 56  uint64  digest of the payload
 *   payloads, each at its offset; the bytes between them are zero.
 * The user blob is the section "user" (owner -1); its size is also in the header.
 * DIGEST of a block of bytes: with the bytes taken as little-endian 32-bit words w_0 .. w_{n-1}, the last one zero-padded,
 *      D = sum_i (uint64(w_i) + 1) * (2 i + 1)   mod 2^64          (numpy: ((w.astype(uint64) + 1) * (2 * arange(n, dtype=uint64) + 1)).sum())
 * The digest of no bytes is 0.  A section whose digest does not match its bytes makes mf_session_load refuse the file.
 * SECTIONS.  In device memory: the MF_STATE_CONTEXT_SECTIONS sections of the context and the MF_STATE_MODEL_SECTIONS sections of every model
 * that mf_state_section_name names ("surfels": the live surfels in mf_download_map's order and layout, whatever shape the buffer has; "pose" /
 * "frame": the device blocks PoseDev / FrameDev; "pose_log": the used entries of the ring, 8 floats each {t xyz, q xyzw, 0}; "vmap_g<level>" / "nmap_g<level>": the model-side
 * pyramid of the last tracking step -- the next step rebuilds it, but an object that only follows the background keeps what it has, and
 * a spawned object inherits the planes of the pool member it is made from, so the pool's planes are sections too, owner = models + position
 * in the pool; "frame_rgb" /
 * "frame_depth" / "frame_mask": the last staged frame, present when it lies in the context's own memory, i.e. not for mf_process_frame_dev /
 * mf_stage_frame_dev, whose buffers belong to the caller).  In host memory: "config" (mf_config), "params" (every read-write key of
 * mf_set_param with its value), "context", "ignore_map_host", "retired" (pose logs of dropped models), "model" (one per model), "user" and,
 * only when the inactive list is not empty, "inactive" (uint32 count, then per entry mf_inactive_info_t and the archive's records; a file
 * without it loads with an empty list).
 * NOT in a session (DESIGN.md lists every member): scratch of the surfel passes, tile and visibility lists, the frame's vertex / normal
 * pyramid and derivative images and the models' Gauss-Newton state (rebuilt by the next frame), timings, profiles, host clocks.
 * ------------------------------------------------------------------------------------------------ */
#define MF_SESSION_VERSION 1
#define MF_STATE_CONTEXT_SECTIONS 14
#define MF_STATE_MODEL_SECTIONS 16
typedef struct mf_session_info_t {
    uint32_t version;
    int32_t width, height;
    int32_t n_models;          /* models in the list */
    int32_t tick;
    uint32_t n_sections;
    int64_t frames;
    uint64_t user_bytes;
    uint64_t file_bytes;
    uint32_t pose_bytes, frame_bytes, run, config_bytes;   /* what the writing build was compiled with */
    int32_t reserved[4];
} mf_session_info_t;
/* Writes the context's session to `path` (through path + ".tmp" and a rename: a failed save leaves no file at `path`, and the context stays
 * usable).  Settles a pending prediction and waits for the context's streams first, as every call does; beyond that it only READS the context:
 * no buffer is compacted, no table rebuilt ("densifyCount", "backgroundRuns" and every later result are what they would have been).
 * user: an opaque blob stored verbatim (may be NULL with user_bytes 0).  MF_EINVAL with the reason in mf_last_error(ctx) when the file cannot
 * be written. */
int mf_session_save(mf_ctx* ctx, const char* path, const void* user, uint64_t user_bytes);
/* Creates a context from a session: mf_create with the saved configuration (on `device` if it is >= 0, else on the saved one), every
 * read-write parameter, the model list in order with its ids and classes, the pool of preallocated models at its saved size, then the
 * sections.  Live surfel buffers come back dense in download order (the first live surfel stays first), with a fresh run table where the
 * saved buffer had a table.  MF_EINVAL with the reason in mf_last_error(NULL) for a short file, a wrong magic or version, a struct size or
 * run length that differs from this build's, or a section whose digest does not match its bytes (the reason names the section); a HIP or
 * allocation failure destroys the half-built context.  *out is NULL unless the call returns MF_OK. */
int mf_session_load(const char* path, int32_t device, mf_ctx** out);
/* The header of a session file and its user blob, without a GPU: checks the magic, the version, the sizes, that the section table and every
 * payload lie inside the file, and the user blob's digest.  user (may be NULL): receives min(user_capacity, blob size) bytes; *user_bytes
 * (may be NULL): the blob's size.  Errors as mf_session_load. */
int mf_session_info(const char* path, mf_session_info_t* out, void* user, uint64_t user_capacity, uint64_t* user_bytes);
/* The digests of the context's device-resident sections, computed on the device without a download: out[0 .. MF_STATE_CONTEXT_SECTIONS) for
 * the context, then MF_STATE_MODEL_SECTIONS words per model in list order; *n = the number of words (MF_EINVAL if capacity is smaller).  Two
 * contexts in the same state give the same words; a dense and a run-structured buffer holding the same surfels give the same "surfels" word. */
int mf_state_digest(mf_ctx* ctx, uint64_t* out, int32_t capacity, int32_t* n);
/* name of section kind i: i < MF_STATE_CONTEXT_SECTIONS a context section, then the MF_STATE_MODEL_SECTIONS per-model kinds; NULL beyond.
 * Word j >= MF_STATE_CONTEXT_SECTIONS of mf_state_digest belongs to model (j - MF_STATE_CONTEXT_SECTIONS) / MF_STATE_MODEL_SECTIONS and has
 * kind MF_STATE_CONTEXT_SECTIONS + (j - MF_STATE_CONTEXT_SECTIONS) % MF_STATE_MODEL_SECTIONS. */
const char* mf_state_section_name(int32_t i);
/* Tooling (tools/session_timing.py): GPU milliseconds between HIP events of ms2[0] k_session_pack over the whole live buffer of `model`, chunk by
 * chunk into the staging block without the copies, and ms2[1] k_state_digest over the same surfels; *surfels: the live count.  Read-only. */
int mf_k_session_timing(mf_ctx* ctx, int32_t model, float* ms2, uint32_t* surfels);

#ifdef __cplusplus
}
#endif
#endif /* MASKFUSION_AMD_H_ */
