// mf_segment.hip -- device half of the multi-model coupling:
//   geometric edge map, threshold, closing, invert   <- Core/Cuda/segmentation.cu:98-177, 217-269, 277-354
//                                                       (MfSegmentation::performSegmentation, MfSegmentation.cpp:149-208)
//   model-ID z-buffer of all models                   <- GlobalProjection::project / downloadDirect
//                                                       (Core/Model/GlobalProjection.cpp:43-114; splat_models.vert,
//                                                        combo_splat_models.frag)
//   object-model pose bookkeeping                     <- Model::updateStaticPose / makeStatic (Core/Model/Model.h:263-264),
//                                                       the 0.2 m jump test of MaskFusion.cpp:268-272
#pragma clang fp contract(off)
#include "mf_device.h"
#include "mf_walk.h"
#include "mf_sprite_device.h"

namespace mf {

// ------------------------------------------------------------------------------------------------
// geometric edge map (concavity + distance terms over the 8 neighbours)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_edge_map(const float* __restrict__ vmap, const float* __restrict__ nmap,
                                                  float* __restrict__ out, int W, int H, float wD, float wC) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int P = W * H, i = y * W + x;
    if (x < 1 || x >= W - 1 || y < 1 || y >= H - 1) { out[i] = 1.0f; return; }
    const float3 v = f3(vmap[i], vmap[P + i], vmap[2 * P + i]);
    const float3 n = f3(nmap[i], nmap[P + i], nmap[2 * P + i]);
    // the reference's invalid vertices carry z = 0; ours carry NaN in every plane
    if (v.z <= 0.0f || isnan(v.z)) { out[i] = 1.0f; return; }
    float c = 0.0f, d = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int ox = (k == 0 || k == 3 || k == 5) ? -1 : ((k == 1 || k == 6) ? 0 : 1);
        const int oy = k < 3 ? -1 : (k < 5 ? 0 : 1);
        const int j = (y + oy) * W + (x + ox);
        const float3 vn = f3(vmap[j], vmap[P + j], vmap[2 * P + j]);
        const float3 nn = f3(nmap[j], nmap[P + j], nmap[2 * P + j]);
        const float dd = dot3(vn - v, n);
        const float ct = (dd < 0) ? 0.f : 1.f - dot3(nn, n);  // getConcavityTerm, segmentation.cu:106-112
        c = fmaxf(ct, c);                                      // fmax drops NaN operands, as in the reference
        d = fmaxf(fabsf(dd), d);                               // getDistanceTerm, :115-119
    }
    c = fmaxf(c, 0.0f) * wC;
    d *= wD;
    out[i] = fminf(1.0f, (c > d) ? c : d);
}

void launch_edge_map(const float* vmap, const float* nmap, float* out, int W, int H, float wD, float wC, hipStream_t s) {
    dim3 grid((W + 63) / 64, (H + 3) / 4);
    hipLaunchKernelGGL(k_edge_map, grid, dim3(256), 0, s, vmap, nmap, out, W, H, wD, wC);
}

// threshold (segmentation.cu:257-262), optionally fused with the final invert (:264-269) when no closing runs
__global__ void k_threshold(const float* __restrict__ in, uint8_t* __restrict__ out, int n, float threshold, int invert) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint8_t v = in[i] > threshold ? 255 : 0;
        out[i] = invert ? (uint8_t)(255 - v) : v;
    }
}
__global__ void k_invert(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = (uint8_t)(255 - in[i]);
}
// dilate_Kernel / erode_Kernel (segmentation.cu:217-255): square window, centre excluded
template <bool kDilate>
__global__ __launch_bounds__(256) void k_morph(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int W, int H, int radius) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    uint8_t r = kDilate ? 0 : 255;
    for (int cy = max(y - radius, 0); cy <= min(y + radius, H - 1); ++cy)
        for (int cx = max(x - radius, 0); cx <= min(x + radius, W - 1); ++cx) {
            if (cy == y && cx == x) continue;
            const uint8_t v = in[cy * W + cx];
            if (kDilate ? v == 255 : v == 0) r = kDilate ? 255 : 0;
        }
    out[y * W + x] = r;
}

// thresholdMap -> morphGeometricSegmentationMap(radius, iterations) -> invertMap; result in `out`, `tmp` is scratch
void launch_edge_binary(const float* edge, uint8_t* out, uint8_t* tmp, int W, int H, float threshold, int radius, int iterations,
                        hipStream_t s) {
    const int n = W * H;
    const int blocks = min((n + 255) / 256, 2048);
    if (iterations <= 0) {
        hipLaunchKernelGGL(k_threshold, dim3(blocks), dim3(256), 0, s, edge, out, n, threshold, 1);
        return;
    }
    dim3 grid((W + 63) / 64, (H + 3) / 4);
    hipLaunchKernelGGL(k_threshold, dim3(blocks), dim3(256), 0, s, edge, out, n, threshold, 0);
    for (int i = 0; i < iterations; ++i) {
        hipLaunchKernelGGL(k_morph<true>, grid, dim3(256), 0, s, out, tmp, W, H, radius);
        hipLaunchKernelGGL(k_morph<false>, grid, dim3(256), 0, s, tmp, out, W, H, radius);
    }
    hipLaunchKernelGGL(k_invert, dim3(blocks), dim3(256), 0, s, out, tmp, n);
    (void)hipMemcpyAsync(out, tmp, n, hipMemcpyDeviceToDevice, s);
}

// ------------------------------------------------------------------------------------------------
// GlobalProjection: the sprite scatter (sprite_scatter_body, mf_sprite_device.h) with global_payload(model order, model id) as the key's
// low word -> LESS on z, earlier model in the list wins ties (GL draw order).  A model dropped by the jump test earlier in this frame
// (pose->alive == 0) draws nothing.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_global_scatter(const SpriteView v, unsigned payload, unsigned long long* __restrict__ keys) {
    if (v.pose->alive == 0) return;
    sprite_scatter_body<1, false>(v, payload, keys, false);
}
// every object model of the list in one launch (grid.z = model; ObjBatch, mf_internal.h): all of them z-test into the one key image
// (f by value, in a function of its own: as obj_splat_scatter, mf_surfel.hip)
__device__ __forceinline__ void obj_global_scatter(const PassFrame f, const PassModel& m, int dense) {
    if (m.pose->alive == 0) return;
    if (dense) sprite_scatter_body<1, false>(global_view(f, m), m.global_payload, f.global_keys, true);
    else sprite_scatter_body<4, false>(global_view(f, m), m.global_payload, f.global_keys, true);
}
__global__ __launch_bounds__(256) void k_obj_global_scatter(const ObjBatch b) { obj_global_scatter(b, b.m[blockIdx.z], b.denseSprites); }
void launch_obj_global_scatter(const ObjBatch& b, int blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_obj_global_scatter, dim3(blocks, 1, b.n), dim3(256), 0, s, b);
}

void launch_global_scatter(const SpriteView& v, unsigned payload, unsigned long long* keys, hipStream_t s, int blocks) {
    hipLaunchKernelGGL(k_global_scatter, dim3(blocks), dim3(256), 0, s, v, payload, keys);
}

__global__ void k_global_resolve(unsigned long long* __restrict__ keys, uint8_t* __restrict__ ids, int P) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const unsigned long long key = keys[p];
        keys[p] = kEmptyKey;
        ids[p] = key == kEmptyKey ? 0 : (uint8_t)(key & 0xFFull);
    }
}
void launch_global_resolve(unsigned long long* keys, uint8_t* ids, int P, hipStream_t s) {
    hipLaunchKernelGGL(k_global_resolve, dim3(min((P + 255) / 256, 2048)), dim3(256), 0, s, keys, ids, P);
}

// ------------------------------------------------------------------------------------------------
// object-model pose bookkeeping (single thread each)
// ------------------------------------------------------------------------------------------------
// spawn: Model::Model (pose = I) + makeStatic(globalPose): initialC2Winv = pose * globalPose^-1 (MaskFusion.cpp:671-684)
__global__ void k_spawn_pose(PoseDev* obj, const PoseDev* bg, FrameDev* objFrame, const FrameDev* bgFrame, PoseDev* host_mirror) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    PoseDev q;
    memset(&q, 0, sizeof(q));
    for (int k = 0; k < 9; ++k) q.R[k] = q.Ri[k] = q.lastR[k] = (k % 4 == 0) ? 1.f : 0.f;
    q.fusionWeight = 1.f;
    q.alive = 1;
    q.weightLiteral = bg->weightLiteral;   // a context-wide switch: the new model inherits it from the background
    m33_inverse_f(bg->R, q.initR);
    const float3 v = mul33(q.initR, f3(bg->t[0], bg->t[1], bg->t[2]));
    q.initT[0] = -v.x; q.initT[1] = -v.y; q.initT[2] = -v.z;
    *obj = q;
    objFrame->tick = bgFrame->tick; objFrame->count = 0; objFrame->countNext = 0; objFrame->phys = 0; objFrame->runs = 0; objFrame->first = 0; objFrame->first_run = 0; objFrame->cover = 0; objFrame->useFillIn = 0; objFrame->done_cover = 0ull;
    MF_FRAME_BBOX_RESET(objFrame);
    objFrame->pad[0] = objFrame->pad[1] = objFrame->pad[2] = 0;
    if (host_mirror) *host_mirror = q;
}
void launch_spawn_pose(PoseDev* obj, const PoseDev* bg, FrameDev* objFrame, const FrameDev* bgFrame, PoseDev* host_mirror, hipStream_t s) {
    hipLaunchKernelGGL(k_spawn_pose, dim3(1), dim3(64), 0, s, obj, bg, objFrame, bgFrame, host_mirror);
}

// Model::updateStaticPose (Model.h:263): overridePose(initialC2Winv * globalPose)
__global__ void k_static_pose(PoseDev* obj, const PoseDev* bg, PoseDev* host_mirror) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    PoseDev p = *obj;
    for (int k = 0; k < 9; ++k) p.lastR[k] = p.R[k];
    for (int k = 0; k < 3; ++k) p.lastT[k] = p.t[k];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            p.R[r * 3 + c] = p.initR[r * 3] * bg->R[c] + p.initR[r * 3 + 1] * bg->R[3 + c] + p.initR[r * 3 + 2] * bg->R[6 + c];
    const float3 t = mul33(p.initR, f3(bg->t[0], bg->t[1], bg->t[2]));
    p.t[0] = t.x + p.initT[0]; p.t[1] = t.y + p.initT[1]; p.t[2] = t.z + p.initT[2];
    pose_derive(p);
    *obj = p;
    if (host_mirror) *host_mirror = p;
}
void launch_static_pose(PoseDev* obj, const PoseDev* bg, PoseDev* host_mirror, hipStream_t s) {
    hipLaunchKernelGGL(k_static_pose, dim3(1), dim3(64), 0, s, obj, bg, host_mirror);
}

// Model::overridePose (Core/Model/Model.h:235-238): lastPose = pose; pose = in  (mode 0: inPose replaces tracking,
// MaskFusion.cpp:413-415) or pose = pose * in (mode 1: bootstrap, :280-283).  in: row-major R, t.
struct PoseArg { float R[9]; float t[3]; };
__global__ void k_override_pose(PoseDev* pose, PoseArg in, int mode, PoseDev* host_mirror) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    PoseDev p = *pose;
    for (int k = 0; k < 9; ++k) p.lastR[k] = p.R[k];
    for (int k = 0; k < 3; ++k) p.lastT[k] = p.t[k];
    if (mode == 0) {
        for (int k = 0; k < 9; ++k) p.R[k] = in.R[k];
        for (int k = 0; k < 3; ++k) p.t[k] = in.t[k];
    } else {
        float R[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R[r * 3 + c] = p.lastR[r * 3] * in.R[c] + p.lastR[r * 3 + 1] * in.R[3 + c] + p.lastR[r * 3 + 2] * in.R[6 + c];
        const float3 t = mul33(p.lastR, f3(in.t[0], in.t[1], in.t[2]));
        for (int k = 0; k < 9; ++k) p.R[k] = R[k];
        p.t[0] = t.x + p.lastT[0]; p.t[1] = t.y + p.lastT[1]; p.t[2] = t.z + p.lastT[2];
    }
    pose_derive(p);
    *pose = p;
    if (host_mirror) *host_mirror = p;
}
void launch_override_pose(PoseDev* pose, const float* in_pose16_colmajor, int mode, PoseDev* host_mirror, hipStream_t s) {
    PoseArg a;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) a.R[r * 3 + c] = in_pose16_colmajor[c * 4 + r];
        a.t[r] = in_pose16_colmajor[12 + r];
    }
    hipLaunchKernelGGL(k_override_pose, dim3(1), dim3(64), 0, s, pose, a, mode, host_mirror);
}

// 16-float per-model record for the multi-GPU gather: R(9) t(3) lastICPError lastICPCount surfels alive
__global__ void k_model_state(const PoseDev* pose, const FrameDev* frame, float* out16) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < 9; ++k) out16[k] = pose->R[k];
    for (int k = 0; k < 3; ++k) out16[9 + k] = pose->t[k];
    out16[12] = pose->lastICPError; out16[13] = pose->lastICPCount; out16[14] = (float)frame->count; out16[15] = (float)pose->alive;
}
void launch_model_state(const PoseDev* pose, const FrameDev* frame, float* out16, hipStream_t s) {
    hipLaunchKernelGGL(k_model_state, dim3(1), dim3(64), 0, s, pose, frame, out16);
}

}  // namespace mf
