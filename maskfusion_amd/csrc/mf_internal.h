// mf_internal.h -- shared declarations of the HIP hot path (gfx950 only; no CPU fallback, no CUDA shims).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mf {

constexpr int kLevels = 3;            // RGBDOdometry::NUM_PYRS (Core/Utils/RGBDOdometry.h:81)
constexpr int kIcpSlots = 32;         // 29 accumulators padded to 32 floats (128 B)
constexpr int kCompactBlocks = 2048;  // fixed grid of the ordered-compaction passes (a VGA map: one 256-element slice per workgroup)
constexpr unsigned long long kEmptyKey = 0xFFFFFFFFFFFFFFFFull;
constexpr int kNoUpdate = 0x7FFFFFFF;

struct Intr {
    float fx, fy, cx, cy;
};

// Device-resident pose block of one model.  Written by kernels only (the Gauss-Newton loop never returns to the
// host); mirrored to pinned host memory at the end of a frame.
struct PoseDev {
    float R[9], t[3];          // model pose (camera -> model frame), row-major
    float Ri[9], ti[3];        // inverse (t_inv uniform of the reference shaders)
    float lastR[9], lastT[3];  // Model::lastPose
    float fusionWeight;        // Model::computeFusionWeight(1.0)
    float lastICPError, lastICPCount;
    float initR[9], initT[3];  // Model::initialC2Winv (objects; Model.h:263-264)
    float incT[3];             // translation of the last tracking increment (MaskFusion.cpp:268)
    int alive;                 // 0 once the 0.2 m jump test dropped the model in this frame
    int rejected;              // 1 if the last tracking step was reverted by the 0.3 m rule (RGBDOdometry.cpp:477-481)
    float lastRGBError, lastRGBCount, lastSO3Error, lastSO3Count;
    int so3Iterations;
    int weightLiteral;         // 1: computeFusionWeight's log map with the reference's float trace ("literalFusionWeight", DESIGN.md finding F5)
    int illIterations;         // Gauss-Newton iterations of the last geometric tracking step whose system was outside the solver's stated domain (GNState::ill)
};

// Result of the SO(3) pre-alignment kernel (RGBDOdometry.cpp:264-324); seeds resultRt of the Gauss-Newton loop.
struct So3Result {
    double R[9];
    float error, count;
    int iterations, pad;
};

// Gauss-Newton state carried from one ICP launch to the next (double-buffered: launch k reads [k-1], block 0 writes [k]).
struct GNState {
    double resultRt[16];       // row-major, RGBDOdometry.cpp:336
    float Rprev[9], tprev[3], Rprev_inv[9];
    float Rcurr[9], tcurr[3];
    float lastICPError, lastICPCount;
    float trR[9], trt[3];      // Isometry3f transform (increment)
    int valid;
    int levelDone;             // pyramid level whose loop was left early (rgbOnly rule, RGBDOdometry.cpp:392-394); -1: none
    float lastRGBError, lastRGBCount;
    int ill;                   // iterations so far whose 6x6 system had fewer than 6 inliers or a pivot below 1e-8 of the largest diagonal entry
                               // (=> cond(A) > 1e8): there the unpivoted fp64 LDL^T here and the reference's pivoted Eigen::LDLT on float-rounded
                               // sums may return different steps (DESIGN.md finding F4); everywhere else they agree to rounding
};

// Scalars that live on the device so that no kernel launch needs a host round trip.
struct FrameDev {
    int tick;                  // MaskFusion::tick
    int count;                 // Model::count (live surfels)
    int countNext;             // snapshot of `count` (dense buffer) / `phys` (sparse buffer) taken by clean pass 1 and read by pass 2, whose last
                               // workgroup then rewrites them (no workgroup of pass 2 reads them, so no intra-launch ordering is assumed)
    int runs;                  // entries of the live buffer's run table (Surfels::box); 0: the buffer is DENSE and has no table -- its surfels are
                               // slots [0, count); > 0: the surfels are the slots [start_r, start_r + len_r) of the runs, in run order (a SPARSE
                               // buffer once a run has lost surfels: Model::clean then works in place, mf_surfel.hip "clean, in place")
    int cover;                 // predicted-colour coverage count (requiresFillIn)
    int useFillIn;             // decision taken for the current tracking step
    int pad[3];
    // Model::lastBoundingBox in millimetres (Model.cpp:315-345; {min xyz, max xyz}, empty = min > max) as of the end of the last frame, and
    // the one being accumulated by this frame's clean pass (object models only; the frame advance moves it over)
    int bbox[6], bbox_acc[6];
    int bbox_tmp[6];           // ... and what the workgroups of a running clean launch have merged so far (empty between launches)
    int phys;                  // first slot behind the last run (= count for a dense buffer): where Model::clean appends the frame's new surfels
    int first;                 // slot of the FIRST live surfel (0 for a dense buffer): the surfel whose vertex id is 0 and which the index map
                               // therefore cannot tell from "no surfel" (index_map.frag writes the id into a texture cleared to 0)
    int runsNext;              // snapshot of `runs` taken by clean pass 1 for pass 2 (like countNext)
    int first_run;             // ... and the run it starts (runs only ever lose surfels: the first non-empty run moves forward, never back)
    unsigned long long done_cover;   // k_splat_tile: (workgroups finished << 32) | coverage count of this launch; zero between launches
};

constexpr int kBBoxEmptyMin = 100000, kBBoxEmptyMax = -100000;   // Model.cpp:315: {1e5, 1e5, 1e5, -1e5, -1e5, -1e5}
constexpr int kBBoxNotRun = 0x7FFFFFFF;   // bbox_acc[0] between the frame advance and the next clean pass: no clean has accumulated a box since
// (device + host) reset of the two boxes of a FrameDev
#define MF_FRAME_BBOX_RESET(f) do { for (int q_ = 0; q_ < 3; ++q_) { (f)->bbox[q_] = (f)->bbox_acc[q_] = (f)->bbox_tmp[q_] = mf::kBBoxEmptyMin; \
                                                                     (f)->bbox[3 + q_] = (f)->bbox_acc[3 + q_] = (f)->bbox_tmp[3 + q_] = mf::kBBoxEmptyMax; } \
                                    (f)->bbox_acc[0] = mf::kBBoxNotRun; } while (0)
// (the box of a frame is the box of its LAST clean pass, like the reference's render pass over the final buffer -- on a spawn frame the spawn
// pass's clean output is not part of it: every clean launch REPLACES bbox_acc with what its workgroups merged into bbox_tmp)
// end of a frame (the GUI's renderPointCloud runs after processFrame, GUI/MainController.cpp:704-717): the accumulated box becomes
// lastBoundingBox; a frame without a clean pass for this model (rgbOnly, model-level calls) leaves the buffer, hence the box, as it was
#define MF_FRAME_BBOX_ADVANCE(f) do { if ((f)->bbox_acc[0] != mf::kBBoxNotRun) for (int q_ = 0; q_ < 6; ++q_) (f)->bbox[q_] = (f)->bbox_acc[q_]; \
                                      (f)->bbox_acc[0] = mf::kBBoxNotRun; } while (0)

struct Surfels {               // SoA of float4, 48 B per surfel in three coalesced streams
    float4* pc;                // position + confidence
    float4* ct;                // colour, unused, initTime, lastTime
    float4* nr;                // normal + radius
    int cap;                   // capacity in surfels (writes beyond it are dropped, like a full transform-feedback buffer)
    // Run table: the buffer as consecutive RUNS of at most kRun slots (after Model::initialise / an uploaded map / a compaction: slots
    // [r kRun, (r + 1) kRun); behind them the runs Model::clean appended, one frame's new surfels after the other), kBoxStride int4 per run:
    //   {enc(min x), enc(min y), enc(min z), enc(newest lastTime)}, {enc(max x), enc(max y), enc(max z), first slot of the run},
    //   {live surfels of the run (they are its FIRST slots, in order), enc(lowest confidence), 1 if a surfel of the run carries lastTime <= 0, 0}
    // (enc: order-preserving float -> int, mf_device.h box_enc).
    // Surfels are stored in creation order, i.e. in spatially coherent runs; a full map is mostly out of view (the 26.5 M-surfel map of
    // configs[4]: 86 %), and the projection passes (index map x 2, prediction, GlobalProjection) only visit the runs whose box meets the viewing
    // frustum and that hold a surfel seen within timeDelta (k_cull) -- the reference streams the whole buffer through every pass
    // (ModelProjection.cpp:100-152,187-268).  Model::clean of a big map visits only the runs in which its tests can change something and
    // compacts each of them where it stands: the order of the surfels (= the reference's transform-feedback order) is the order of the runs.
    int4* box;
};
constexpr int kRun = 512;
constexpr int kBoxStride = 3;
__host__ __device__ inline int run_start(const int4* box, int r) { return box[kBoxStride * r + 1].w; }
__host__ __device__ inline int run_len(const int4* box, int r) { return box[kBoxStride * r + 2].x; }
struct VisList { const int* list; const int* count; };   // device memory: run indices (any order) and how many (launch_cull)
constexpr int kBoxEmptyMin = 0x7FFFFFFF, kBoxEmptyMax = (int)0x80000000;

// Persistent per-model block of the tracker (device memory, written once when the model is created): what the batched
// Gauss-Newton kernels need to find a model's maps, state and partial sums from blockIdx alone.
struct TrackModelDev {
    const float4* predV; const float4* predN;    // prediction consumed by initICPModel
    PoseDev* pose; PoseDev* pose_host; const FrameDev* frame;
    float* vm[3]; float* nm[3];                   // model-side vertex / normal pyramid (global frame)
    float* partials[2]; GNState* st;              // ping-pong per-workgroup partial sums [nb][32]; st[0], st[1]
    float* log;                                   // [19][32] reduced systems (background model) or nullptr
    double* trace;                                // [20][kGnTraceRow] Gauss-Newton trace (mf_gn_device.h: gn_trace_write) or nullptr
    float jump_limit;                             // object models: 0.2 m rule of MaskFusion.cpp:268-272; background: 0
    int allow_fill;                               // Model::allowsFillIn (background only)
    int* rect;                                    // {x0, y0, x1, y1}: the pixels of nm[0] that hold a normal (an object's prediction is NaN outside the object,
                                                  // Q3; the coarser levels' normals lie inside it shifted by the level) -- written by the batched model
                                                  // pyramid for object models, read by the batched pixel pass (slab culling), re-armed {INT_MAX, INT_MAX,
                                                  // INT_MIN, INT_MIN} by the batched finalize
};
constexpr int kMaxTrackBatch = 32;
constexpr int kGnTraceRow = 64;
struct TrackBatch { const TrackModelDev* m[kMaxTrackBatch]; int n; };   // by value in the kernel arguments

// ---------------- preprocessing ----------------
void launch_bilateral_model_pyramid(const float* depth, float* depthF, const float4* predV, const float4* predN, const float* fillDepth,
                                    const FrameDev* frame, const PoseDev* pose, float* const vmaps[3], float* const nmaps[3], int W, int H, Intr k,
                                    hipStream_t s);   // the filter + launch_model_pyramid's work in one launch (mf_model_pyramid.hip)
void launch_bilateral(const float* depth, float* out, int W, int H, hipStream_t s);
void launch_pyrdown_f(const float* src, float* dst, int sw, int sh, hipStream_t s);
void launch_vmap_nmap(const float* depth, float* vmap, float* nmap, int W, int H, Intr k, float cutoff, hipStream_t s);
// depth pyramid (2 x pyrDownGaussF) + vertex/normal maps of the three levels in one launch; k: level-0 intrinsics
void launch_frame_pyramid(const float* depth, float* const vmap[3], float* const nmap[3], int W, int H, Intr k, float cutoff,
                          hipStream_t s);

// launch_frame_pyramid's and launch_model_pyramid's work (device pose) in one launch (mf_model_pyramid.hip: k_frame_model_pyramid)
void launch_frame_model_pyramid(const float* depthF, float* const fvmap[3], float* const fnmap[3], float cutoff, const float4* predV, const float4* predN,
                                const float* fillDepth, const FrameDev* frame, const PoseDev* pose, float* const vmaps[3], float* const nmaps[3], int W, int H,
                                Intr k, hipStream_t s, int* fixup = nullptr);   // fixup: as launch_model_pyramid's

// Fused RGBDOdometry::initICPModel (mf_model_pyramid.hip).  pose: device PoseDev (R,t used).  fill-in inputs may be null (no fill-in).
void launch_model_pyramid(const float4* predV, const float4* predN, const float* fillDepth, const FrameDev* frame,
                          const PoseDev* pose, const float* R9t3_host_or_null, float* const vmaps[3],
                          float* const nmaps[3], int W, int H, Intr k, hipStream_t s, int* fixup = nullptr);
// fixup ("tilePyramid"): the tile pass has already written the pyramid without fill-in -- the launch runs only if frame->useFillIn is set, and then
// counts the frame in *fixup

// ---------------- odometry (mf_odometry.hip; the parts of a Gauss-Newton step: mf_gn_device.h) ----------------
// One Gauss-Newton iteration: [reduce+solve of the previous launch] -> normal equations of this level.
struct IcpLaunch {
    const float* vmap_curr; const float* nmap_curr; const float* vmap_prev; const float* nmap_prev;
    int W, H; Intr k;
    float distThres, angleThres;
    const float* partials_in; int nblocks_in;   // previous launch (nullptr/0 for the first)
    float* partials_out;
    const GNState* state_in; GNState* state_out;
    float* log_out;                              // optional [32] floats of the reduced system solved in this launch
    double* trace = nullptr; int it = 0;         // optional: the model's Gauss-Newton trace ([20][kGnTraceRow]) and this launch's iteration index
    unsigned long long* prof_out = nullptr;      // optional [16] shader-clock stamps (workgroup 0)
    const PoseDev* pose_in = nullptr;            // first launch only: seed the Gauss-Newton state from this pose
    const So3Result* so3_in = nullptr;           // first launch only: SO(3) pre-alignment seeds resultRt's rotation
};
int icp_grid_blocks(int W, int H);       // workgroups of the RGB-D iteration kernels for this level
int icp_geo_grid_blocks(int W, int H);   // workgroups of the geometric kernel k_icp_iter (more of them at the coarse levels: one pixel slot per thread)
// the launch form of k_icp_iter for a level: threads per workgroup, pixel slots per thread, workgroups, pixels per workgroup (chunk), and how many
// of the workgroups hold at least one pixel (chunks round up to 64 pixels, so the last workgroups of a capped grid can lie past the image)
struct IcpForm { int threads, slots, blocks, chunk, live; };
IcpForm icp_launch_form(int W, int H);
void launch_icp_iteration(const IcpLaunch& a, hipStream_t s);
// ---- the same loop for SEVERAL models at once (MaskFusion.cpp:247-276 tracks them one after the other): one launch serves
// iteration k of every tracked model.  Split in two kernels per iteration -- "solve" (one workgroup per model: reduce the
// previous iteration's partials, LDL^T, pose) and "pixels" (grid.y = model, no prologue, any number of workgroup rounds) --
// because the redundant per-workgroup prologue of k_icp_iter would be paid once per model and per round.
int icp_batch_max_blocks(int W, int H);                       // upper bound of workgroups per model of launch_icp_batch_pixels
int icp_batch_blocks(int W, int H, int n_models);             // workgroups per model it will use for this image size
void launch_model_pyramid_batch(const TrackBatch& b, const float* fillDepth, int W, int H, Intr k, hipStream_t s);   // (mf_model_pyramid.hip, as the next)
void launch_bilateral_model_pyramid_batch(const float* depth, float* depthF, const TrackBatch& b, const float* fillDepth, int W, int H, Intr k,
                                          hipStream_t s);   // the depth filter + launch_model_pyramid_batch's work in one launch
// it = 0 seeds the states from the model poses (+ SO(3) rotation); it >= 1 finishes iteration it-1 whose pixel pass used nb_in blocks
void launch_icp_batch_solve(const TrackBatch& b, int it, int nb_in, const So3Result* so3_or_null, hipStream_t s);
// The pyramid level a pixel pass works on.  row_z: launch_row_zrange's output for this level (nullptr: no culling -- every workgroup walks its pixels)
struct IcpBatchLevel { int level; const float* vmap_curr; const float* nmap_curr; int W, H; Intr k; float distThres, angleThres; const float2* row_z; };
// fused: launch_icp_batch_solve(b, it, nb_in, so3) is this launch's prologue
void launch_icp_batch_pixels(const TrackBatch& b, int it, const IcpBatchLevel& l, bool fused, int nb_in, const So3Result* so3_or_null, hipStream_t s);
// depth range of every row of the frame's three vertex maps: out[0 .. H) level 0, [H .. H + H/2) level 1, [.. + H/4) level 2: {min z, max z} over the
// row's valid vertices ({+inf, -inf}: none)
void launch_row_zrange(const float* const vmap[3], int W, int H, float2* out, hipStream_t s);
// last solve (iteration n_it - 1) + Model pose / lastPose / statistics / jump rule
void launch_icp_batch_finalize(const TrackBatch& b, int n_it, int nb_in, const So3Result* so3_or_null, hipStream_t s);
// What the end of a tracking step writes, for the three finalize kernels (the batched one fills it per model from the TrackModelDev): the pose block
// and its pinned mirror (or nullptr), optionally the last reduced system ([32] floats), the pre-alignment that seeded the step (its statistics go to
// the pose), optionally the trace and the iterations that ran.  jump_limit > 0: object-model rule of MaskFusion.cpp:268-272 (|increment| > limit => alive = 0)
struct GnFinalize { PoseDev* pose; PoseDev* host_mirror; float* log; float jump_limit; const So3Result* so3; double* trace; int n_it; };
// What the last iteration of a step left for the finalize step to finish: its per-workgroup partial sums and the state it started from; with the
// photometric term also the RGB partials, the correspondence counts and its pyramid level (else unused)
struct GnLast { const float* partials; int nblocks; const GNState* state; const float* rgb_partials; const int2* cnt; int level; };
// Last reduce+solve, then pose / lastPose / inverse / fusion weight update and host mirror.
void launch_icp_finalize(const GnLast& last, const GnFinalize& f, hipStream_t s);
// Stand-alone icpStep (parity tests): host-provided poses, output 32 floats.
void launch_icp_step_standalone(const float* Rcurr, const float* tcurr, const float* vc, const float* nc,
                                const float* Rpi, const float* tprev, Intr k, const float* vp, const float* np,
                                float distThres, float angleThres, int W, int H, float* partials, GNState* st2,
                                float* out32, hipStream_t s);
// The same through k_icp_batch_pixels (form 1; form 2: with slab culling against rect4, host {x0, y0, x1, y1}) or k_rgbd_iter (form 3).  dpose: device
// Rcurr[9] tcurr[3] Rprev_inv[9] tprev[3].  Own scratch, synchronous; 0, -1 (no memory) or -2 (HIP error).
int icp_step_form_standalone(int form, const float* dpose, const float* vc, const float* nc, Intr k, const float* vp, const float* np, float distThres,
                             float angleThres, int W, int H, const int* rect4, float* out32, hipStream_t s);

struct RgbCorr { int16_t u0, v0; float diff; };  // DataTerm (types.cuh:75-81) packed to 8 B; u0 < 0: no correspondence

struct RgbLevel {  // one pyramid level of RGBDOdometry's photometric inputs
    const int16_t* dIdx; const int16_t* dIdy;          // nextdIdx / nextdIdy
    const float* lastDepth; const float* nextDepth;    // Q1: both come from the model prediction
    const uint8_t* lastImage; const uint8_t* nextImage;
    int W, H;
    float minScale;        // minimumGradientMagnitudes[level]^2 / sobelScale^2
    float maxDepthDelta;   // 0.07
    const uint8_t* gate;   // optional: 1 where the iteration-independent tests of RGBResidual pass (border, 4x4 window of the
                           // next image > 0, gradient magnitude), written once per frame by the derivative kernel; nullptr =
                           // evaluate them per pixel
};

// ---------------- photometric term + SO(3) (mf_rgbd.hip, mf_odometry.hip) ----------------
void launch_intensity(const uint8_t* img, int channels, uint8_t* dst, int n, hipStream_t s);
void launch_pyrdown_u8(const uint8_t* src, uint8_t* dst, int sw, int sh, hipStream_t s);
void launch_derivative(const uint8_t* src, int16_t* dx, int16_t* dy, int W, int H, float minScale, uint8_t* gate /*or null*/, hipStream_t s);
// up to three independent small image jobs in ONE launch (mf_rgbd.hip): kind 0 pyrDownUcharGauss (W, H = source size), 1 pyrDownGaussF (source size),
// 2 computeDerivativeImages (+ gate image; W, H = image size)
struct SmallJob { int kind; const void* src; void* dst; void* dst2; uint8_t* gate; int W, H; float minScale; };
struct SmallJobs { SmallJob j[3]; int n; };
void launch_small_jobs(const SmallJobs& a, hipStream_t s);
// intensity pyramid (3 levels) + derivative / gate images of a frame in one launch; false (nothing launched) for sizes its tiling does not cover
bool launch_rgb_pyramid(const uint8_t* rgb, int W, int H, uint8_t* const gray[3], int16_t* const dIdx[3], int16_t* const dIdy[3], uint8_t* const gate[3],
                        const float minScale[3], bool derivatives, hipStream_t s);
// level 0 of a model's "last" depth / intensity pyramids (populateRGBDData of initRGBModel; Q1: initRGB re-uses the depth)
// frameToFrameRGB != 0 (and a fill-in image given): initRGBModel takes the fill-in image whatever the fill-in decision (Model.cpp:399-400)
void launch_rgbd_last_l0(const float4* predV, const float* fillDepth, const uint8_t* predGray, const uint8_t* fillGray,
                         const FrameDev* frame, float* depth0, uint8_t* image0, int n, hipStream_t s, int frameToFrameRGB = 0);
// scratch: so3_scratch_bytes(W2, H2) of device memory; any image size (at most 512 workgroups, which stride over a larger image).
// Returns 0, or -1 if nothing was launched (*out is then not written and must not be used as a seed)
size_t so3_scratch_bytes(int W2, int H2);
int launch_so3_prealign(const uint8_t* lastImage2, const uint8_t* nextImage2, int W2, int H2, Intr k2, So3Result* out, void* scratch,
                        hipStream_t s);
void launch_rgb_residual_only(const RgbLevel& L, const float* krk_kt, RgbCorr* corres, int* sums, hipStream_t s);
void launch_rgb_step_only(const RgbLevel& L, const RgbCorr* corres, float sigma, Intr k, float sobelScale, double* out32, hipStream_t s);
// One RGB-D Gauss-Newton iteration = two launches (see mf_odometry.hip)
struct RgbdLaunch {
    IcpLaunch icp;
    RgbLevel L;
    RgbCorr* corres;
    const float* rgb_partials_in; float* rgb_partials_out;
    const int2* cnt_in; int2* cnt_out;
    float icpWeight; int icpOn; int rgbOnly; float sobelScale;
    int level, prev_level;
    const So3Result* so3_in;
};
void launch_rgbd_iteration(const RgbdLaunch& l, hipStream_t s);
void launch_rgbd_finalize(const GnLast& last, float icpWeight, int icpOn, int rgbOnly, const GnFinalize& f, hipStream_t s);

// ---------------- surfels ----------------
void launch_init_surfels(const uint8_t* rgb, const float* depthRaw, const float* depthF, int W, int H, Intr k,
                         float maxDepth, const FrameDev* frame, float4* rec /*[P][3]*/, uint8_t* flags, hipStream_t s);
// Grid of the four grid-stride surfel kernels below: 2048 workgroups by default; a model that is known to be small (an object model
// of a few thousand surfels) may be launched with fewer -- the loops are grid-stride, the result does not depend on the grid.
constexpr int kSurfelGridBlocks = 2048;
// ---- the arguments of a frame's surfel passes: index map, data association, update, second index map, clean, prediction ----
// Each pass exists as a launch for ONE model (mf_frame.inl: enqueue_fuse_clean, mf_model_api.inl) and as a launch for ALL object models of a
// frame (grid.z = model, mf_surfel.hip: k_obj_*); both forms describe their work with the same three structs, filled by the same functions
// (mf_frame.inl: pass_frame, pass_model), and build every kernel-argument struct from them with the builders below.
// The per-model scratch of the passes.  The context owns one set, shared by the model-by-model launches (the reference's per-model passes never
// overlap in time); an object model that takes part in the batched launches brings its own (mf_context.hip: alloc_surfel_scratch knows the sizes).
struct SurfelScratch {
    unsigned long long* keys;                         // [P] z-test key image, kEmptyKey between passes
    int* index; float4* ivc; float4* inr;             // [P] row-major index map of the pass that feeds fuse
    float4* ict;                                      // [P] its colorTime image -- the shared set only: nullptr for an object model's own
    float4* iclean;                                   // [2 P] packed column-major index map of the pass that feeds clean: 2 x float4 per texel (the spare
                                                      // word carries the filtered depth), or one float4 per texel (16-byte taps, "cleanTap16") in its first half
    uint8_t* cand_op; float4* cand_rec;               // [P], [3 P] the frame's candidates (association pass)
    int* upd_first;                                   // [capacity] winning merge candidate per surfel, kNoUpdate between passes
    int* cand_best;                                   // [P] surfel a merge candidate was associated with (fuse_data -> fuse_update)
    int* clean_ctl;                                   // [kCleanCtlInts] k_clean_runs' finished-workgroup counter, zero between launches
    uint8_t* flags; float* newconf; int* block_counts;   // [capacity + P] x 2, [kCompactBlocks]: the two-launch clean form's intermediates
};
// What the passes of a frame share, whichever model they serve
struct PassFrame {
    int W, H; Intr k; float maxDepthProcessed, globalMaxDepth; int timeDelta; float outlierCoeff;
    int cleanLiteral;                  // the clean window walked with the shader's own fp32 trip count
    int bboxLimit;                     // object models limit their fusion depth by lastBoundingBox ("objectBoundingBoxLimit")
    int fuseLanes;                     // lanes per candidate of the association pass: 1 or 4
    int cleanTapGroup;                 // 16-byte taps requested together: 1, 3 (a window column) or 9 ("cleanTapGroup")
    const uint8_t* rgb; const float* depthRaw; const float* depthF; const uint8_t* mask; const PoseDev* bg_pose;
    uint8_t* maskT;                    // the mask in column-major order, beside the packed maps (every model's resolve writes the same bytes)
    float* depthT;                     // != nullptr: the packed maps hold 16-byte taps, and this plane the filtered depth in column-major order (as maskT)
    unsigned long long* global_keys;   // GlobalProjection's key image (the shared set's)
};
// What a model brings to them
struct PassModel {
    Surfels a, b;                      // live buffer when the frame's fusion starts / the other one (small models: fuse a -> b, clean b -> a; from
                                       // inPlaceElements on: fuse in place in a, clean a -> b, then b is live; big ones: everything in place in a)
    FrameDev* frame; PoseDev* pose;
    int maskID; float confThreshold, fuseMaxDepth, weightMultiplier;
    SurfelScratch scr;                 // the shared set (a model handled on its own) or the model's own (the batch)
    int* host_count;                   // pinned mirror of the surfel count
    unsigned long long* host_append; unsigned clean_seq;   // in place: pinned mirror of where the buffer ends after THIS clean pass, tagged with the pass's
                                                           // sequence number (append_mirror() below); nullptr: none
    float4* predV; float4* predN; uchar4* predImage; uint16_t* predTime; uint8_t* predGray;
    FrameDev* host_frame; float* log_slot;
    unsigned global_payload;           // GlobalProjection: global_payload(position in the model list, id)
};
// The surfel passes of ALL object models of a frame, one launch per pass (grid.z = model).  An object model holds a few thousand surfels: each of
// its ~11 per-frame launches is pure launch latency (~85 us per object and frame in round 2's profile).  The batched kernels are the single-model
// kernels' bodies called with the frame's arguments and one model's, picked from a device array by blockIdx.z.  One launch has one form:
struct ObjBatch : PassFrame {
    const PassModel* m; int n;
    int denseSprites;                  // 1: a model of the batch is above inPlaceElements -- the sprite passes (prediction, GlobalProjection) run one thread
                                       // per surfel: such a map holds sub-pixel sprites, and four lanes per surfel repeat its set-up four times
    int updateCopy;                    // 1: every model of the batch is below inPlaceElements -- update.vert as a copy a -> b, clean b -> a
    int cleanSmall;                    // 1: the two-launch clean form src -> dst; 0: every model of the batch has a run table -- clean in place
};

// The launches below take the key image, maps and records from m.scr, the size, limits and frame planes from f; their key images are column-major
// (index_scatter_one; the batched object kernels scatter row-major).
// vis: nullptr = every surfel; else the runs launch_cull found possibly visible
void launch_index_scatter(Surfels src, const PassFrame& f, const PassModel& m, hipStream_t s, int blocks = kSurfelGridBlocks, const VisList* vis = nullptr);
// run table of a DENSE buffer s (slots [0, frame->count)): fixed runs of kRun slots (after Model::initialise / an uploaded map / a compaction; the
// in-place clean pass maintains it afterwards).  refresh: s has a table -- only the entries' contents are recomputed from the surfels
void launch_run_table(Surfels s, FrameDev* frame, hipStream_t st, bool refresh = false);
size_t run_table_runs(long capacity, long pixels);      // runs a buffer's table can hold (the host compacts the buffer before they run out)
size_t run_table_entries(long capacity, long pixels);   // int4 entries of that table (kBoxStride per run)
// the runs of s whose box meets the viewing frustum (image bounds + 2 px, -1 cm .. maxDepth + 1 cm) and that hold a surfel seen within
// timeDelta: their indices -> list (any order), their number -> count[0]; ctl: 2 ints, zero between launches
void launch_cull(Surfels s, const FrameDev* frame, const PoseDev* pose, int W, int H, Intr k, float maxDepth, int timeDelta, int* list, int* count,
                 int* ctl, int max_runs, hipStream_t st);
// The index-map resolve's outputs.  Two consumers, two shapes: index + vertConf + normRad (+ colorTime) as row-major images for the pass that feeds
// fuse, ONE packed record per texel, column-major, for the pass that feeds clean (mf_surfel.hip: "Two consumers, two output shapes").
// Frame planes that travel with the packed map (copy_unstable.vert:139-156 looks the filtered depth and the mask up at the surfel's own texel: in the
// packed, column-major order these are neighbours of its window taps; in the row-major images every lane pulled a sector of its own):
// depthF -> the packed record's spare word (32-byte record) or depthT (16-byte tap: column-major floats), mask -> maskT (column-major bytes)
struct ResolveOut {
    int* index; float4* vc; float4* nr; float4* ct; float4* packed; const float* depthF; const uint8_t* mask; uint8_t* maskT;
    float* depthT; float tapThreshold;    // tap16: the 16-byte tap (one float4 per texel), live against this confidence threshold; depthT: its depth plane
    const FrameDev* frame;    // the buffer's frame state (`first`)
    // with `packed`, optional: what Model::clean's mask-disagreement rule (copy_unstable.vert:139-156) can meet in this frame, for the run culling of
    // the in-place clean (k_cull_clean): order-preserving ints -- {min, max} filtered depth over the texels of the LEFT column, the RIGHT column, the
    // TOP row, the BOTTOM row whose mask is foreign to the model (neither its id nor >= 255), then the min over ALL foreign texels (kDecayStats
    // ints); armed (empty) between frames
    int* decay_stats; int maskID;
    // packed: one float4 per texel (tap16_encode) instead of the 32-byte record.  The frame planes travel in depthT / maskT -- unless both are
    // nullptr: a frame without a mask, for the background ("maskFreeClean": clean_test<.., kMaskFree = true> reads neither)
    int tap16;
};
// the row-major maps; want_ct: the colorTime image too (only the clean pass of a freshly spawned model and the model API read it from there)
__host__ __device__ inline ResolveOut resolve_out_maps(const PassModel& m, bool want_ct) {
    ResolveOut o{};
    o.index = m.scr.index; o.vc = m.scr.ivc; o.nr = m.scr.inr; o.ct = want_ct ? m.scr.ict : nullptr; o.frame = m.frame;
    return o;
}
// the packed map: the 32-byte record with the filtered depth in its spare word, or (f.depthT) the 16-byte tap {x, y, z', initTime} (z' = NaN unless
// index > 0, confidence > the model's threshold and z > 0, sign bit = lastTime == tick) -- only for a clean pass enqueued with it, with the same
// tick and threshold.  maskFree (16-byte taps only): every byte of the mask is the model's id (a frame without a mask, for the background) -- no
// plane is carried and no texel is foreign: depthT / maskT and the statistics are not touched ("maskFreeClean").
// decay_stats (optional): kDecayStats ints for launch_cull_clean (armed by launch_arm_decay_stats / k_cull_clean)
__host__ __device__ inline ResolveOut resolve_out_packed(const PassFrame& f, const PassModel& m, bool maskFree = false, int* decay_stats = nullptr) {
    ResolveOut o{};
    const bool planes = !(f.depthT && maskFree);
    o.packed = m.scr.iclean; o.depthF = f.depthF; o.mask = f.mask; o.maskT = planes ? f.maskT : nullptr; o.depthT = planes ? f.depthT : nullptr;
    o.tapThreshold = m.confThreshold; o.frame = m.frame; o.decay_stats = planes ? decay_stats : nullptr; o.maskID = m.maskID; o.tap16 = f.depthT ? 1 : 0;
    return o;
}
void launch_index_resolve_maps(Surfels src, const PassFrame& f, const PassModel& m, bool want_ct, hipStream_t s);
void launch_index_resolve_packed(Surfels src, const PassFrame& f, const PassModel& m, hipStream_t s, bool maskFree = false, int* decay_stats = nullptr);

struct FuseDataArgs {
    const uint8_t* rgb; const float* depthRaw; const float* depthF; const uint8_t* mask; int maskID;
    const FrameDev* frame; const PoseDev* pose; float weightMultiplier; float maxDepth;
    int bboxLimit;                 // 1: object models limit their fusion depth by lastBoundingBox (upstream with its GUI; "objectBoundingBoxLimit")
    int W, H; Intr k;
    const int* index; const float4* vc; const float4* nr;
    uint8_t* cand_op; float4* cand_rec; int* upd_first;
    int* cand_best;                // surfel a merge candidate was associated with (read by the update pass; untouched for the others)
};
__host__ __device__ inline FuseDataArgs fuse_data_args(const PassFrame& f, const PassModel& m) {
    FuseDataArgs a;
    a.rgb = f.rgb; a.depthRaw = f.depthRaw; a.depthF = f.depthF; a.mask = f.mask; a.maskID = m.maskID; a.frame = m.frame; a.pose = m.pose;
    a.weightMultiplier = m.weightMultiplier; a.maxDepth = m.fuseMaxDepth; a.bboxLimit = f.bboxLimit; a.W = f.W; a.H = f.H; a.k = f.k;
    a.index = m.scr.index; a.vc = m.scr.ivc; a.nr = m.scr.inr;
    a.cand_op = m.scr.cand_op; a.cand_rec = m.scr.cand_rec; a.upd_first = m.scr.upd_first; a.cand_best = m.scr.cand_best;
    return a;
}
void launch_fuse_data(const FuseDataArgs& a, int lanes /* per candidate: 1 or 4 (a quad shares the 3 x 3 window, one column per lane) */, hipStream_t s);
// update.vert IN PLACE: one thread per candidate, the winning candidate of a surfel (upd_first) merges into it where it stands
void launch_fuse_update(Surfels s, const PassFrame& f, const PassModel& m, hipStream_t st);
// the same as a copy src -> dst over the whole buffer; scatter: the index-map scatter of the pass that feeds clean rides on it (the form for small maps)
struct IndexScatterArgs { const PoseDev* pose; int W, H; Intr k; float maxDepth; int timeDelta; unsigned long long* keys; int transposed; };
__host__ __device__ inline IndexScatterArgs index_scatter_args(const PassFrame& f, const PassModel& m, bool scatter, int transposed) {
    IndexScatterArgs ix;
    ix.pose = m.pose; ix.W = f.W; ix.H = f.H; ix.k = f.k; ix.maxDepth = f.maxDepthProcessed; ix.timeDelta = f.timeDelta;
    ix.keys = scatter ? m.scr.keys : nullptr; ix.transposed = transposed;
    return ix;
}
void launch_fuse_update_copy(Surfels src, Surfels dst, const PassFrame& f, const PassModel& m, bool scatter, hipStream_t s, int blocks = kSurfelGridBlocks);
// seq (20 bits) | runs of the table (18 bits) | first slot behind the last run (26 bits): one 64-bit store the host can read at any time --
// its bounds on what the device has appended then start from a recent exact value instead of the last compaction (mf_frame.inl: prepare_in_place)
constexpr int kAppendSeqBits = 20, kAppendRunBits = 18, kAppendPhysBits = 26;
__host__ __device__ inline unsigned long long append_mirror(unsigned seq, int runs, int phys) {
    return ((unsigned long long)(seq & ((1u << kAppendSeqBits) - 1u)) << (kAppendRunBits + kAppendPhysBits)) | ((unsigned long long)(unsigned)runs << kAppendPhysBits) |
           (unsigned long long)(unsigned)phys;
}
// Model::clean (copy_unstable.vert:53-157, Model.cpp:649-772).  What every form of the pass is given: the shader's uniforms and textures + the frame's candidates (new-surfel records of the association pass)
// + the two-launch form's intermediates.  Element i < count is an old surfel, element count + c is candidate c (only op == 2 live).
struct CleanArgs {
    Surfels src, dst; FrameDev* frame; const PoseDev* pose; int W, H; Intr k;
    int timeDelta; float confThreshold; float outlierCoeff; int maskID; int transposed;
    int literal;   // 1: the window is walked with copy_unstable.vert's own fp32 induction variable (4 or 5 steps per axis), 0: 4 x 4
    const int* index; const float4* vc; const float4* ct;   // separate images (only when the packed map is absent)
    const float4* packed;                                    // {vertConf | initTime, lastTime, index, 0} per texel
    const float* depthF; const uint8_t* mask;
    const uint8_t* maskT;                                    // the mask in the packed map's order (only with `packed`)
    const float* depthT;                                     // the filtered depth in the same order (only with the 16-byte tap, unless maskFree)
    const uint8_t* cand_op; const float4* cand_rec;
    uint8_t* flags; float* newconf;    // keep flag / new confidence per element: pass 1 -> pass 2 of the two-launch form
    int* block_counts;                 // [kCompactBlocks] survivors per workgroup (two-launch form)
    int* host_count;
    unsigned long long* host_append; unsigned seq;   // append: PassModel::host_append / clean_seq
    int append;                        // two-launch form, 1: the buffer's own surfels have been cleaned where they stand (k_clean_runs) -- the two passes
                                       // handle the frame's candidates only and append the survivors at frame->phys (dst = src)
    const int* run_list; const int* run_count;   // k_clean_runs: the runs to visit (k_cull_clean); nullptr: every run of the table
    int* ctl;                          // k_clean_runs: kCleanCtlInts ints, zero between launches
    int tap16;                         // `packed` holds 16-byte taps (clean_test<true>)
    int tapGroup;                      // 16-byte taps requested together: 1 (one by one), 3 (a window column) or 9 (the window) -- "cleanTapGroup"
    int maskFree;                      // 1: the frame has no mask and the model is id 0: no mask / depth planes travel with the taps -- "maskFreeClean"
};
// The pass that reads the packed column-major map a resolve pass of the SAME enqueue wrote (resolve_out_packed: the same f, m and maskFree), every run.
// maskFree: an object model's mask is never its own id everywhere -- only the background's launches pass it.
__host__ __device__ inline CleanArgs clean_args(const PassFrame& f, const PassModel& m, Surfels src, Surfels dst, int append, bool maskFree = false) {
    CleanArgs a;
    a.src = src; a.dst = dst; a.frame = m.frame; a.pose = m.pose; a.W = f.W; a.H = f.H; a.k = f.k; a.timeDelta = f.timeDelta;
    a.confThreshold = m.confThreshold; a.outlierCoeff = f.outlierCoeff; a.maskID = m.maskID; a.transposed = 1; a.literal = f.cleanLiteral;
    a.index = m.scr.index; a.vc = m.scr.ivc; a.ct = m.scr.ict; a.packed = m.scr.iclean;
    a.depthF = f.depthF; a.mask = f.mask; a.maskT = f.maskT; a.depthT = maskFree ? nullptr : f.depthT;
    a.cand_op = m.scr.cand_op; a.cand_rec = m.scr.cand_rec; a.flags = m.scr.flags; a.newconf = m.scr.newconf; a.block_counts = m.scr.block_counts;
    a.host_count = m.host_count; a.host_append = m.host_append; a.seq = m.clean_seq;
    a.append = append; a.run_list = nullptr; a.run_count = nullptr; a.ctl = m.scr.clean_ctl;
    a.tap16 = f.depthT ? 1 : 0; a.tapGroup = f.cleanTapGroup; a.maskFree = maskFree ? 1 : 0;
    return a;
}
// two launches (flags + ordered copy), a.src -> a.dst: dst is a DENSE buffer without a run table.  src must be dense.
int compact_blocks_for(long elements);   // workgroups of an ordered-compaction launch for that many elements (<= kCompactBlocks)
void launch_clean_small(const CleanArgs& a, hipStream_t s, int blocks = kCompactBlocks);
// IN PLACE (mf_surfel.hip "clean, in place"; a.src = a.dst has a run table): launch_clean_runs tests the surfels of the listed runs (nullptr: of
// every run) and compacts each run where it stands; launch_clean_append tests the frame's candidates and appends the survivors behind the last run.
// blocks: clean_runs_grid(elements expected)
constexpr int kCleanGridMax = 2048;
constexpr int kCleanCtlInts = 8;
int clean_runs_grid(long elements);
void launch_clean_runs(CleanArgs a, const VisList* runs, int blocks, hipStream_t s);
void launch_clean_append(CleanArgs a, hipStream_t s);
// the runs launch_clean_runs has to visit for the BACKGROUND-style culling of a model: those in which one of the pass's rules can apply at all
// (decay_stats: launch_index_resolve_packed's, re-armed here; list / count / ctl as launch_cull)
constexpr int kDecayStats = 9;     // ResolveOut::decay_stats (mf_surfel.hip): {min, max} x {left, right, top, bottom border} + min over all foreign texels
void launch_arm_decay_stats(int* stats /*[kDecayStats]*/, hipStream_t st);   // once, when the statistics block is allocated
void launch_cull_clean(Surfels s, const FrameDev* frame, const PoseDev* pose, int W, int H, Intr k, int timeDelta, float confThreshold, int* decay_stats,
                       int* list, int* count, int* ctl, int max_runs, hipStream_t st);
// compaction of a sparse buffer: the surfels of src's runs -> dst, dense (no table); offs: scratch of run_table_runs() + 1 ints
void launch_densify(Surfels src, Surfels dst, FrameDev* frame, int* offs, int* host_count, hipStream_t st);
// its first step on its own (k_run_offsets): offs[r] = live surfels before run r, offs[runs] = all of them; *total (optional) = the live surfels of the
// buffer, with or without a table
void launch_run_offsets(Surfels s, const FrameDev* frame, int* offs, int* total, hipStream_t st);
// generic ordered compaction of [n_dev] records (3 x float4 each, record-major) -> surfels, sets frame->count
void launch_compact_records(const float4* rec, const uint8_t* flags, int n, Surfels dst, FrameDev* frame,
                            int* block_counts, int* host_count_mirror, hipStream_t s);
// ---- the sprite passes: the prediction (combinedPredict) and GlobalProjection, each as a scatter form (mf_surfel.hip, mf_segment.hip) and a tiled
// form (mf_splat.hip); the arithmetic all four share is mf_sprite_device.h ----
// What a sprite pass draws: a model's live buffer seen through its pose, with the gates of splat.vert / splat_models.vert
struct SpriteView { Surfels src; FrameDev* frame; const PoseDev* pose; int W, H; Intr k; float maxDepth, confThreshold; int timeDelta; };
constexpr float kGlobalConfThreshold = 12.0f;   // GlobalProjection::project draws with a fixed confidence threshold (GlobalProjection.cpp:43)
__host__ __device__ inline SpriteView sprite_view(const PassFrame& f, const PassModel& m, float maxDepth, float confThreshold) {
    SpriteView v;
    v.src = m.a; v.frame = m.frame; v.pose = m.pose; v.W = f.W; v.H = f.H; v.k = f.k; v.maxDepth = maxDepth; v.confThreshold = confThreshold;
    v.timeDelta = f.timeDelta;
    return v;
}
__host__ __device__ inline SpriteView predict_view(const PassFrame& f, const PassModel& m) { return sprite_view(f, m, f.maxDepthProcessed, m.confThreshold); }
__host__ __device__ inline SpriteView global_view(const PassFrame& f, const PassModel& m) { return sprite_view(f, m, f.globalMaxDepth, kGlobalConfThreshold); }
// low word of GlobalProjection's keys: LESS on z, then the earlier model of the list (GL draw order); the resolve pass reads the id
__host__ __device__ inline unsigned global_payload(int order, int id) { return ((unsigned)order << 8) | ((unsigned)id & 255u); }
// What the prediction writes.  rgb / predGray / fillGray may be null: the intensity images of the NEXT tracking step's photometric term;
// fillPassthrough: fill_rgb.frag's `passthrough` (frameToFrameRGB, Model.cpp:981) -- the fill-in image is the raw frame everywhere.
// The builder is the object batch's; a model drawn on its own adds the fill-in image (mf_frame.inl: pred_out_one)
struct PredOut { float4* predV; float4* predN; uchar4* predImage; uint16_t* predTime; const uint8_t* rgb; uint8_t* predGray; uint8_t* fillGray; int fillPassthrough; };
__host__ __device__ inline PredOut pred_out(const PassFrame& f, const PassModel& m) {
    return PredOut{m.predV, m.predN, m.predImage, m.predTime, f.rgb, m.predGray, nullptr, 0};
}
void launch_splat_scatter(const SpriteView& v, unsigned long long* keys, hipStream_t s, int blocks = kSurfelGridBlocks);
void launch_splat_resolve(const SpriteView& v, unsigned long long* keys, const PredOut& out, hipStream_t s);   // leaves the key image empty; counts v.frame->cover
void launch_global_scatter(const SpriteView& v, unsigned payload, unsigned long long* keys, hipStream_t s, int blocks = kSurfelGridBlocks);   // nothing if the model is not alive
// Tiled form of scatter + resolve (mf_splat.hip): bins surfels to 16-pixel-wide tiles, z-test in LDS, writes the maps (the prediction) or merges
// the tile's winners into the key image (GlobalProjection) directly.
size_t splat_tiles_scratch_ints(int W, int H);
struct SplatTuning { int sprite_lanes = 4, tile_threads = 512, tile_h = 24; };   // A/B knobs of the tile passes ("spriteLanes", "tileThreads", "tileHeight"), owned by the context
// The context's scratch of the tile passes (mf_frame.inl: tile_lists).  tile_count [tiles] must be zero on the first call (it is left zero);
// entries [tiles][entries_cap / tiles]; rec0, rec1, bbox (8 B each) [surfels]: the sprite set-up the binning pass keeps for the tile pass
struct TileLists { int* tile_count; int* entries; int entries_cap; float4* rec0; float4* rec1; void* bbox; SplatTuning tune; };
// The launch shape of the tile passes for an image: tiles of 16 x tileH pixels, lanes per sprite, threads per tile workgroup.  fits: the LDS
// histograms of the binning pass hold that many tiles (else the passes take their scatter form)
struct TileShape { int tilesX, tilesY, tileH, lanes, threads; bool fits; };
TileShape splat_tile_shape(int W, int H, SplatTuning tune);
inline bool splat_tiled_applies(int W, int H, SplatTuning tune) { return splat_tile_shape(W, H, tune).fits; }   // the tiled launches would not return -1
// The end-of-frame bookkeeping (k_frame_advance: pose log entry, fill-in decision for the next tracking step, tick++, host mirror) as
// the epilogue of the tiled prediction: its last workgroup to finish runs it, one launch less per model and frame.
struct FrameAdvance { FrameDev* host_mirror; const PoseDev* bg_pose; float* log_slot; };
// filter (optional): the NEXT frame's depth filter (launch_bilateral(depth, out, W, H)), enqueued with the binning pass: in its launch (fused != 0,
// k_bin_bilateral) or as a launch of its own between the binning pass and the tile pass.  The two read and write nothing in common.
struct SplatFilterJob { const float* depth; float* out; int fused; };
// pyramid (optional, "tilePyramid"): every tile workgroup also writes the three levels of the model-side pyramid of its tile (vm / nm: launch_model_pyramid's
// planes; the model pose is the view's), as launch_model_pyramid computes them WITHOUT fill-in -- a frame whose fill-in decision comes out 1 needs that launch
// behind.  frame_depth != nullptr ("fusedTilePyramid"): launch_frame_pyramid(frame_depth, frame_vmap, frame_nmap, W, H, k, frame_cutoff)'s work rides in
// the same launch, in workgroups of its own behind the tile workgroups.  The tile pass and that pyramid read and write nothing in common.
struct SplatPyramidJob { float* vm[3]; float* nm[3]; const float* frame_depth; float* frame_vmap[3]; float* frame_nmap[3]; float frame_cutoff; };
// What may ride on the tiled prediction, each optional (nullptr): the end-of-frame bookkeeping, the two jobs above, and "splatProfile"'s
// [tiles][8] shader-clock stamps
struct SplatRiders { const FrameAdvance* advance; const SplatFilterJob* filter; const SplatPyramidJob* pyramid; unsigned long long* prof; };
// vis: nullptr = every surfel; else the runs launch_cull found possibly visible.  Both return -1 (nothing launched) if the image does not fit
int launch_splat_tiled(const SpriteView& v, const TileLists& lists, const PredOut& out, const SplatRiders& riders, const VisList* vis, hipStream_t s);
int launch_global_tiled(const SpriteView& v, const TileLists& lists, unsigned payload, unsigned long long* keys, const VisList* vis, hipStream_t s);
// ---- the surfel passes of ALL object models of a frame, one launch per pass (struct ObjBatch above) ----
void launch_obj_global_scatter(const ObjBatch& b, int blocks, hipStream_t s);          // GlobalProjection of every object model (mf_segment.hip)
void launch_obj_fuse_clean(const ObjBatch& b, int blocks, int clean_blocks, hipStream_t s, int compact_blocks = kCompactBlocks);   // predictIndices -> fuse -> predictIndices -> clean
void launch_obj_predict_advance(const ObjBatch& b, int blocks, hipStream_t s);         // combinedPredict (scatter form) + the end-of-frame bookkeeping
void launch_fill_keys(unsigned long long* keys, int n, hipStream_t s);
void launch_fill_int(int* p, int v, int n, hipStream_t s);
// ---------------- multi-model coupling (mf_segment.hip) ----------------
void launch_edge_map(const float* vmap, const float* nmap, float* out, int W, int H, float wD, float wC, hipStream_t s);
void launch_edge_binary(const float* edge, uint8_t* out, uint8_t* tmp, int W, int H, float threshold, int radius,
                        int iterations, hipStream_t s);
void launch_global_resolve(unsigned long long* keys, uint8_t* ids, int P, hipStream_t s);
int gn_solve_standalone(const double* sys29, const double* resultRt16, const float* Rprev9, const float* tprev3, double* x_serial, double* x_wave,
                        double* resultRt_out, float* Rcurr9, float* tcurr3, float* stats2, hipStream_t s);
void launch_spawn_pose(PoseDev* obj, const PoseDev* bg, FrameDev* objFrame, const FrameDev* bgFrame, PoseDev* host_mirror,
                       hipStream_t s);
void launch_static_pose(PoseDev* obj, const PoseDev* bg, PoseDev* host_mirror, hipStream_t s);
void launch_override_pose(PoseDev* pose, const float* in_pose16_colmajor, int mode, PoseDev* host_mirror, hipStream_t s);
void launch_model_state(const PoseDev* pose, const FrameDev* frame, float* out16, hipStream_t s);

// ---------------- headless rendering (mf_render.hip) ----------------
constexpr int kMaxRenderModels = 256;
struct RenderModel {                  // one drawn model, in draw order (device array; M is filled by the render's first launch)
    Surfels s; const FrameDev* frame; const PoseDev* pose;
    unsigned base;                    // draw index of slot 0: {depth, base + slot} is the z-test key
    int max_runs;                     // entries of the render's cull grid for this model (runs of its table, or chunks of kRun slots)
    float thr; int class_id, color_type, index, is_background;
    float M[12];                      // model -> view, row-major 3 x 4
};
struct RenderView { float Vi[12]; };  // world -> view, row-major 3 x 4
struct RenderArgs {
    RenderModel* models; int n_models;
    int W, H; Intr k; float near_z, far_z;
    int drawUnstable, drawPoints, drawWindow, timeDelta;
    const FrameDev* tick_frame;       // the background's frame state: `time` of the shaders
    const float* palette; int n_palette;
    uchar4 clear;
    int* work; int* work_count;       // the runs k_render_cull listed: model << 24 | run; their number (zero on entry)
    int tilesX, tilesY, tile_cap;
    int* tile_count;                  // [tiles], zero on entry
    uint2* entries;                   // [tiles][tile_cap] {draw index, tile-local box}
    int* overflow;                    // set when a tile's list ran over its slice (pinned host memory)
    uchar4* out_rgba; float* out_depth; int* out_model;
};
void launch_render(RenderArgs a, const RenderView& v, const PoseDev* bg_pose, int max_runs, hipStream_t s);

// ---------------- run evaluation: fixed-radius nearest neighbour (mf_eval.hip) ----------------
uint64_t nn_workspace_bytes(int64_t n_target);
// the reason of the calling thread's last failed call that takes no context (mf_mesh.hip), or null: what mf_last_error(NULL) returns
const char* cloud_last_error();
// records who + text as that reason and returns rc (mf_mesh.hip's and mf_eval_trimesh.hip's failures)
int cloud_fail(const char* who, const char* text, int rc);
// the whole of mf_cloud_nn_dev (include/maskfusion_amd.h): grid build + query on stream s, then a synchronisation of s; *why (why may be null): the reason of an error, untouched when there is none
int nn_run(const float* d_target, int target_stride, int64_t n_target, const float* d_query, int query_stride, int64_t n_query,
           const float* T16 /*host, column-major, or null*/, float radius, float* d_dist, int32_t* d_idx, void* d_ws, uint64_t ws_bytes, hipStream_t s,
           const char** why);
// a model's live surfels in download order (offs: launch_run_offsets): their positions -> out[n], NaN for confidence <= thr
void launch_nn_gather(Surfels s, const FrameDev* frame, const int* offs, float thr, float4* out, int n, int max_runs, hipStream_t st);

// ---------------- sessions (mf_session.hip) ----------------
// the live surfels with ordinals [first, first + n) of download order -> out[0, 3 n): 48-byte records, mf_download_map's layout (offs:
// launch_run_offsets; first + n at most its total).  Reads s, its table and frame->runs; writes out only
void launch_session_pack(Surfels s, const FrameDev* frame, const int* offs, int first, int n, float4* out, hipStream_t st);
// the inverse into a DENSE buffer: rec[0, 3 n) -> slots [first, first + n) of dst's three streams
void launch_session_unpack(const float4* rec, int n, Surfels dst, int first, hipStream_t st);
// *word += sum_i (uint64(w_i) + 1) (2 (first_word + i) + 1) mod 2^64 over the little-endian 32-bit words of data[0, bytes) (tail zero-padded;
// data 16-byte aligned, device memory).  The digest of a block is what this leaves in a zeroed word; blocks of one section add up
void launch_state_digest(const void* data, uint64_t bytes, uint64_t first_word, unsigned long long* word, hipStream_t st);
// ... of the records launch_session_pack would write for the whole buffer (*total live surfels, device memory: launch_run_offsets' total;
// expected: a host-side guess that sizes the grid)
void launch_state_digest_surfels(Surfels s, const FrameDev* frame, const int* offs, const int* total, int expected, unsigned long long* word,
                                 hipStream_t st);
uint64_t state_digest_host(const void* data, uint64_t bytes, uint64_t first_word = 0);   // the same word for host memory

// end-of-frame bookkeeping: tick++, cover -> useFillIn decision for the next frame
// ... and the pose-log entry of this frame (MaskFusion.cpp:580-596) when log != nullptr
void launch_pose_log(const PoseDev* pose, const PoseDev* bg_pose /*nullptr: the background itself*/, float* slot, hipStream_t s);
void launch_frame_advance(FrameDev* frame, int W, int H, FrameDev* host_mirror, const PoseDev* pose, const PoseDev* bg_pose,
                          float* log_slot, hipStream_t s);

}  // namespace mf
