// mf_model_pyramid.hip -- RGBDOdometry::initICPModel (Core/Utils/RGBDOdometry.cpp:153-185: copyMaps, resizeVMap/NMap, tranformMaps;
// Core/Cuda/cudafuncs.cu:207-331,366-445) + FillIn (Core/Shaders/fill_*.frag) as one pass over the prediction, and the launches that run it
// beside the frame's depth filter or the frame's own pyramid.  The arithmetic is in mf_model_pyramid_device.h, shared with the tile pass.
#include <string.h>

#include "mf_internal.h"
#include "mf_device.h"
#include "mf_bilateral_device.h"
#include "mf_frame_pyramid_device.h"
#include "mf_model_pyramid_device.h"

namespace mf {

// ------------------------------------------------------------------------------------------------
// Model-side pyramid: copyMaps + resize x2 + transform x3 (+ fill-in) in ONE pass.  One thread owns a 4x4 block of
// level-0 pixels = 2x2 of level 1 = 1 pixel of level 2, so the averages follow the reference's operation order
// ((x00 + x01 + x10 + x11) / 4, level 2 from level-1 values) and nothing is re-read from HBM.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ MapPx load_model_px(const float4* __restrict__ predV, const float4* __restrict__ predN,
                                               const float* __restrict__ fillDepth, bool useFill, int x, int y, int W,
                                               int H, Intr k) {
    const int p = y * W + x;
    float4 v4 = predV[p], n4 = predN[p];
    if (useFill) {
        if (v4.z == 0) {  // fill_vertex.frag:37-53
            const float z = fillDepth[p];
            v4 = make_float4(((float)x - k.cx) * z * (1.0f / k.fx), ((float)y - k.cy) * z * (1.0f / k.fy), z, 1.f);
        }
        if (n4.z == 0) {  // fill_normal.frag:34-50
            const float3 vp = get_vertex(fillDepth, W, H, x, y, (float)x, (float)y, k);
            const float3 n = get_normal_forward(fillDepth, W, H, x, y, vp, k);
            n4 = make_float4(n.x, n.y, n.z, 1.f);
        }
    }
    return copy_maps_px(v4, n4);   // copyMapsKernel, cudafuncs.cu:286-305
}

// (mul33_fixed, store_tx, the quad broadcasts and the two smaller levels' arithmetic: mf_model_pyramid_device.h, shared with the tile pass's epilogue)
struct PyrArgs {
    const float4* predV; const float4* predN; const float* fillDepth; const FrameDev* frame; const PoseDev* pose;
    float R[9]; float t[3]; int hostPose;
    float* vm[3]; float* nm[3];
    int W, H; Intr k;
    TrackBatch b;   // b.n > 0: grid.z = model, everything but fillDepth / W / H / k comes from the model's block
    int* fixup;     // non-null ("tilePyramid"): the tile pass has written the no-fill pyramid -- run only if frame->useFillIn, and count such frames here
};

// One thread per LEVEL-1 pixel (2x2 level-0 pixels); the four lanes of a DPP quad hold the 2x2 level-1 block of one level-2
// pixel and exchange their values with quad broadcasts, so the averages keep the reference's operation order
// ((x00 + x01 + x10 + x11) / 4, level 2 from level-1 values).  (A thread per level-2 pixel -- 19 200 threads walking 16
// pixels each -- left three quarters of the CUs idle: 15 us.)
__device__ __forceinline__ void model_pyramid_body(const PyrArgs& a0, const int blk_x, const int blk_y, const int blk_z) {
    PyrArgs a = a0;
    if (a0.b.n > 0) {
        const TrackModelDev* __restrict__ md = a0.b.m[blk_z];
        a.predV = md->predV; a.predN = md->predN; a.frame = md->frame; a.pose = md->pose; a.hostPose = 0;
        a.fillDepth = md->allow_fill ? a0.fillDepth : nullptr;
#pragma unroll
        for (int i = 0; i < 3; ++i) { a.vm[i] = md->vm[i]; a.nm[i] = md->nm[i]; }
    }
    const int W2 = a.W >> 2, H2 = a.H >> 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane & 3, bx = b & 1, by = b >> 1;
    const int x2 = blk_x * 16 + (lane >> 2);
    const int y2 = blk_y * 4 + wave;
    const bool inside = x2 < W2 && y2 < H2;   // whole quads are in or out: the DPP exchanges below stay well defined
    float R[9]; float3 t;
    if (a.hostPose) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = a.R[k];
        t = f3(a.t[0], a.t[1], a.t[2]);
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = a.pose->R[k];
        t = f3(a.pose->t[0], a.pose->t[1], a.pose->t[2]);
    }
    const bool useFill = a.fillDepth != nullptr && a.frame != nullptr && a.frame->useFillIn != 0;
    const int W = a.W, H = a.H, W1 = W >> 1, H1 = H >> 1;
    const int P0 = W * H, P1 = W1 * H1, P2 = W2 * H2;

    bool n0any = false;                       // (batched tracker) this thread's level-0 pixels that hold a normal: their box
    int n0x0 = 0, n0y0 = 0, n0x1 = 0, n0y1 = 0;
    MapPx px[4];
    if (inside) {
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = 4 * x2 + 2 * bx + dx, y = 4 * y2 + 2 * by + dy;
                px[dy * 2 + dx] = load_model_px(a.predV, a.predN, a.fillDepth, useFill, x, y, W, H, a.k);
                store_tx(a.vm[0], a.nm[0], P0, y * W + x, px[dy * 2 + dx].v, px[dy * 2 + dx].vok, px[dy * 2 + dx].n,
                         px[dy * 2 + dx].nok, R, t);
                if (px[dy * 2 + dx].nok) {
                    n0x0 = n0any ? min(n0x0, x) : x; n0y0 = n0any ? min(n0y0, y) : y; n0x1 = n0any ? max(n0x1, x) : x; n0y1 = n0any ? max(n0y1, y) : y;
                    n0any = true;
                }
            }
    }
    // levels 1 and 2 (mf_model_pyramid_device.h; executed by every lane: its quad broadcasts need them active)
    model_pyramid_down(px, inside, b, R, t, a.vm[1], a.nm[1], P1, (2 * y2 + by) * W1 + 2 * x2 + bx, a.vm[2], a.nm[2], P2, y2 * W2 + x2);
    if (a0.b.n > 0 && !a0.b.m[blk_z]->allow_fill) {
        // batched tracker, object models: the rectangle of level-0 pixels that hold a normal (TrackModelDev::rect) -- a superset of the pixels store_tx
        // wrote a normal to (it writes NaN wherever the flag is off), which is all the pixel pass of the Gauss-Newton loop can pair a frame pixel
        // with.  A level-1 / level-2 normal needs all four normals below it (resizeMapKernel), so the rectangle shifted right by the level bounds
        // those levels too.  An object covers ~1 % of the image: nearly every wavefront sees no normal at all and leaves after one ballot.
        if (__ballot(inside && n0any) != 0ull) {
            int* __restrict__ rect = a0.b.m[blk_z]->rect;
            const bool on = inside && n0any;
            const int x0 = wave_min_i(on ? n0x0 : 0x7FFFFFFF), y0 = wave_min_i(on ? n0y0 : 0x7FFFFFFF);
            const int x1 = wave_max_i(on ? n0x1 : (int)0x80000000), y1 = wave_max_i(on ? n0y1 : (int)0x80000000);
            if (lane == 0) { atomicMin(&rect[0], x0); atomicMin(&rect[1], y0); atomicMax(&rect[2], x1); atomicMax(&rect[3], y1); }
        }
    }
}

// "tilePyramid": the tile pass of the fused head has already written the three levels without fill-in (mf_splat.hip: k_splat_tile's epilogue), and its
// last workgroup has decided frame->useFillIn behind them -- the kernel boundary orders that write.  A launch with a.fixup set only repairs the
// frames whose decision came out "fill": every workgroup leaves at once otherwise; else the launch runs as ever and overwrites all three levels, and
// its first workgroup counts the frame ("pyramidFixupFrames").  true: this workgroup has nothing to do.
__device__ __forceinline__ bool pyramid_fixup_skips(const PyrArgs& a, const bool first) {
    if (a.fixup == nullptr) return false;
    if (a.frame->useFillIn == 0) return true;
    if (first && threadIdx.x == 0) *a.fixup += 1;
    return false;
}

__global__ __launch_bounds__(256) void k_model_pyramid(const PyrArgs a) {
    if (pyramid_fixup_skips(a, blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)) return;
    model_pyramid_body(a, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
}

// The depth filter of the frame and the model-side pyramid of the same frame's tracking step in ONE launch ("fusedPreprocessLaunch"): the two are
// independent -- the filter reads the new depth image, the pyramid the previous frame's prediction -- and complement each other (the filter is
// VALU-bound on 1 208 workgroups at VGA, the pyramid a 20 MB stream on 300), but on one stream two launches run one after the other.  Workgroups
// below nbil run bilateral_body (mf_bilateral_device.h), the others model_pyramid_body with their index as the 2-D block of k_model_pyramid:
// the same instructions on the same data as the two kernels, hence the same bits.
// (six wavefronts per SIMD = six workgroups per compute unit: at VGA all 1 508 workgroups are resident at once; the pyramid half would take 83 registers)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_bilateral_model_pyramid(const float* __restrict__ depth, float* __restrict__ out, int W, int H, int nbil,
                                                                 int interleave, const PyrArgs a) {
    __shared__ float tile[kBLdsH * kBLdsW];
    // Which half a workgroup belongs to.  Workgroups are dispatched in index order: with the filter's first and the pyramids' behind them, a launch
    // that does not fit the GPU at once (1280 x 960: 4 808 + 1 200 per tracked model) ran the two halves one after the other.  The pyramids' workgroups
    // are therefore spread evenly among the filter's (a Bresenham walk: workgroup b is a pyramid workgroup when floor((b + 1) npyr / total) steps),
    // so that the VALU-bound half and the bandwidth-bound half are in flight together from the first round on.
    const int gx = ((W >> 2) + 15) / 16, gy = ((H >> 2) + 3) / 4, per = gx * gy;
    // (a launch that IS resident at once -- VGA, one tracked model: 1 508 workgroups -- keeps the filter's workgroups first: their index is what
    // places a tile on the XCD that holds its neighbours' halo rows, worth 1 us there)
    const int total = (int)gridDim.x, npyr = total - nbil, b = (int)blockIdx.x;
    int before, after;
    if (interleave) { before = (int)(((long long)b * npyr) / total); after = (int)(((long long)(b + 1) * npyr) / total); }
    else { before = b < nbil ? 0 : b - nbil; after = b < nbil ? 0 : b - nbil + 1; }
    if (after == before) { bilateral_body(depth, out, W, H, tile, b - before, (int)threadIdx.x, true); return; }
    // (a.b.n > 0: the batched tracker's pyramids, model by model -- k_model_pyramid's grid.z unrolled)
    const int j = before;
    model_pyramid_body(a, (j % per) % gx, (j % per) / gx, j / per);
}

void launch_model_pyramid(const float4* predV, const float4* predN, const float* fillDepth, const FrameDev* frame,
                          const PoseDev* pose, const float* R9t3_host_or_null, float* const vmaps[3], float* const nmaps[3],
                          int W, int H, Intr k, hipStream_t s, int* fixup) {
    PyrArgs a;
    a.predV = predV; a.predN = predN; a.fillDepth = fillDepth; a.frame = frame; a.pose = pose;
    a.fixup = fixup;
    a.hostPose = R9t3_host_or_null != nullptr;
    for (int i = 0; i < 9; ++i) a.R[i] = a.hostPose ? R9t3_host_or_null[i] : 0.f;
    for (int i = 0; i < 3; ++i) a.t[i] = a.hostPose ? R9t3_host_or_null[9 + i] : 0.f;
    for (int i = 0; i < 3; ++i) { a.vm[i] = vmaps[i]; a.nm[i] = nmaps[i]; }
    a.W = W; a.H = H; a.k = k;
    a.b.n = 0;
    dim3 grid(((W >> 2) + 15) / 16, ((H >> 2) + 3) / 4);
    hipLaunchKernelGGL(k_model_pyramid, grid, dim3(256), 0, s, a);
}

void launch_bilateral_model_pyramid(const float* depth, float* depthF, const float4* predV, const float4* predN, const float* fillDepth,
                                    const FrameDev* frame, const PoseDev* pose, float* const vmaps[3], float* const nmaps[3], int W, int H, Intr k,
                                    hipStream_t s) {
    PyrArgs a;
    a.predV = predV; a.predN = predN; a.fillDepth = fillDepth; a.frame = frame; a.pose = pose;
    a.fixup = nullptr;
    a.hostPose = 0;
    for (int i = 0; i < 9; ++i) a.R[i] = 0.f;
    for (int i = 0; i < 3; ++i) a.t[i] = 0.f;
    for (int i = 0; i < 3; ++i) { a.vm[i] = vmaps[i]; a.nm[i] = nmaps[i]; }
    a.W = W; a.H = H; a.k = k;
    a.b.n = 0;
    const int nbil = bilateral_grid(W, H), npyr = (((W >> 2) + 15) / 16) * (((H >> 2) + 3) / 4);
    hipLaunchKernelGGL(k_bilateral_model_pyramid, dim3(nbil + npyr), dim3(256), 0, s, depth, depthF, W, H, nbil, (nbil + npyr > 1536) ? 1 : 0, a);
}

// ... and for the batched tracker: the filter beside launch_model_pyramid_batch's work
void launch_bilateral_model_pyramid_batch(const float* depth, float* depthF, const TrackBatch& b, const float* fillDepth, int W, int H, Intr k,
                                          hipStream_t s) {
    PyrArgs a;
    memset(&a, 0, sizeof(a));
    a.fillDepth = fillDepth; a.W = W; a.H = H; a.k = k; a.b = b;
    const int nbil = bilateral_grid(W, H), npyr = (((W >> 2) + 15) / 16) * (((H >> 2) + 3) / 4) * b.n;
    hipLaunchKernelGGL(k_bilateral_model_pyramid, dim3(nbil + npyr), dim3(256), 0, s, depth, depthF, W, H, nbil, (nbil + npyr > 1536) ? 1 : 0, a);
}

// The frame's pyramid and the model-side pyramid of the same tracking step in ONE launch ("fusedFramePyramids"), for a frame whose prediction was
// deferred into its successor's head (mf_frame.inl: enqueue_fused_head): there the model-side pyramid can no longer ride beside the depth filter --
// the prediction it reads is drawn behind the filter --, and both pyramids are streams that wait for nothing but the tile pass.  The first nfp
// workgroups run frame_pyramid_body (mf_frame_pyramid_device.h: every operation rounded on its own), the others model_pyramid_body with their index
// as k_model_pyramid's 2-D block: the same instructions on the same data as the two kernels, hence the same bits.  Both counts are multiples of 8
// and a launch that is not resident at once interleaves the halves in groups of 8 workgroups, so that a frame tile's index keeps the XCD that holds
// its neighbours (xcd_contiguous_tile) either way.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_frame_model_pyramid(const FramePyrArgs f, int nfp, int interleave, const PyrArgs a) {
    __shared__ float lds[kFpLdsFloats];
    const int groups = (int)gridDim.x >> 3, gpyr = groups - (nfp >> 3), g = (int)blockIdx.x >> 3, lane = (int)blockIdx.x & 7;
    int before, after;   // pyramid groups in front of group g / of group g + 1 (a Bresenham walk, as k_bilateral_model_pyramid's)
    if (interleave) { before = (int)(((long long)g * gpyr) / groups); after = (int)(((long long)(g + 1) * gpyr) / groups); }
    else { before = g < (nfp >> 3) ? 0 : g - (nfp >> 3); after = g < (nfp >> 3) ? 0 : before + 1; }
    if (after == before) { frame_pyramid_body(f, lds, ((g - before) << 3) + lane); return; }
    const int gx = ((a.W >> 2) + 15) / 16, gy = ((a.H >> 2) + 3) / 4, j = (before << 3) + lane;
    if (j >= gx * gy) return;   // (padding of the pyramid half to a multiple of 8)
    if (pyramid_fixup_skips(a, j == 0)) return;
    model_pyramid_body(a, j % gx, j / gx, 0);
}

void launch_frame_model_pyramid(const float* depthF, float* const fvmap[3], float* const fnmap[3], float cutoff, const float4* predV, const float4* predN,
                                const float* fillDepth, const FrameDev* frame, const PoseDev* pose, float* const vmaps[3], float* const nmaps[3], int W, int H,
                                Intr k, hipStream_t s, int* fixup) {
    FramePyrArgs f;
    f.depth = depthF; f.W = W; f.H = H; f.k = k; f.cutoff = cutoff;
    for (int i = 0; i < 3; ++i) { f.vmap[i] = fvmap[i]; f.nmap[i] = fnmap[i]; }
    PyrArgs a;
    a.predV = predV; a.predN = predN; a.fillDepth = fillDepth; a.frame = frame; a.pose = pose;
    a.fixup = fixup;
    a.hostPose = 0;
    for (int i = 0; i < 9; ++i) a.R[i] = 0.f;
    for (int i = 0; i < 3; ++i) a.t[i] = 0.f;
    for (int i = 0; i < 3; ++i) { a.vm[i] = vmaps[i]; a.nm[i] = nmaps[i]; }
    a.W = W; a.H = H; a.k = k;
    a.b.n = 0;
    const int nfp = xcd_padded_grid(frame_pyramid_tiles(W, H)), npyr = xcd_padded_grid((((W >> 2) + 15) / 16) * (((H >> 2) + 3) / 4));
    // (six 256-thread workgroups per compute unit: 1 536 are resident at once, as for k_bilateral_model_pyramid)
    hipLaunchKernelGGL(k_frame_model_pyramid, dim3(nfp + npyr), dim3(256), 0, s, f, nfp, (nfp + npyr > 1536) ? 1 : 0, a);
}

void launch_model_pyramid_batch(const TrackBatch& b, const float* fillDepth, int W, int H, Intr k, hipStream_t s) {
    PyrArgs a;
    memset(&a, 0, sizeof(a));
    a.fillDepth = fillDepth; a.W = W; a.H = H; a.k = k; a.b = b;
    dim3 grid(((W >> 2) + 15) / 16, ((H >> 2) + 3) / 4, b.n);
    hipLaunchKernelGGL(k_model_pyramid, grid, dim3(256), 0, s, a);
}

}  // namespace mf
