// mf_preproc.hip -- per-frame image preprocessing on plain HBM arrays.
//   bilateral depth filter   <- MaskFusion::filterDepth + depth_bilateral_metric.frag (Core/MaskFusion.cpp:650-657)
//   depth pyramid            <- pyrDownGaussF (Core/Cuda/cudafuncs.cu:333-364, 510-532)
//   vertex + normal maps     <- createVMap + createNMap (Core/Cuda/cudafuncs.cu:109-205), fused into one pass
// every float op individually rounded in this file (the preprocessing feeds normals, which amplify 1-ulp depth
// differences ~1000x; keeping these maps within rounding of a plain reading of the reference keeps parity tight).
// BEFORE the header: its inline helpers (cross3, dot3, normalized_rsqrt) are compiled under whatever is in force where they are
// DEFINED -- until round 3 the pragma sat below the include, createNMap's cross product was fused, and the normal maps differed from
// the restatement's in the last bit on hardware only (the CPU-executed build has contraction off everywhere): 0.03-0.2 % of the label
// pixels of the 8-object scene.
#pragma clang fp contract(off)
#include "mf_device.h"
#include "mf_bilateral_device.h"
#include "mf_frame_pyramid_device.h"

namespace mf {

// 13x13 bilateral: the body lives in mf_bilateral_device.h (shared with the launch that runs it beside the model-side pyramid)
__global__ __launch_bounds__(256) void k_bilateral(const float* __restrict__ depth, float* __restrict__ out, int W, int H) {
    __shared__ float tile[kBLdsH * kBLdsW];
    bilateral_body(depth, out, W, H, tile, (int)blockIdx.x, (int)threadIdx.x, true);
}

void launch_bilateral(const float* depth, float* out, int W, int H, hipStream_t s) {
    hipLaunchKernelGGL(k_bilateral, dim3(bilateral_grid(W, H)), dim3(256), 0, s, depth, out, W, H);
}

// ------------------------------------------------------------------------------------------------
// 5x5 Gaussian half-sampling that skips NaNs, with the reference's border quirk: the upper loop
// bounds clamp to cols-1 / rows-1 exclusive and the kernel is indexed from the far corner.
// ------------------------------------------------------------------------------------------------
// (gauss5, the binomial row, lives in mf_frame_pyramid_device.h)
__global__ __launch_bounds__(256) void k_pyrdown_f(const float* __restrict__ src, float* __restrict__ dst, int sw, int sh) {
    const int dw = sw >> 1, dh = sh >> 1;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    const int tx = min(2 * x + 3, sw - 1);
    const int ty = min(2 * y + 3, sh - 1);
    float sum = 0.f;
    int count = 0;
    for (int cy = max(0, 2 * y - 2); cy < ty; ++cy) {
        for (int cx = max(0, 2 * x - 2); cx < tx; ++cx) {
            const float v = src[cy * sw + cx];
            if (!isnan(v)) {
                const float w = gauss5(ty - cy - 1) * gauss5(tx - cx - 1);
                sum += v * w;
                count += (int)w;
            }
        }
    }
    dst[y * dw + x] = sum / (float)count;
}

void launch_pyrdown_f(const float* src, float* dst, int sw, int sh, hipStream_t s) {
    const int dw = sw / 2, dh = sh / 2;
    dim3 grid((dw + 63) / 64, (dh + 3) / 4);
    hipLaunchKernelGGL(k_pyrdown_f, grid, dim3(256), 0, s, src, dst, sw, sh);
}

// ------------------------------------------------------------------------------------------------
// Vertex map and normal map of one level in one pass: the three vertices a normal needs are recomputed from
// depth (bitwise the values createVMap stores), so the normal never waits for a vertex-map round trip.
// Planar SoA [3][H][W] outputs keep the ICP loads of 64 consecutive lanes on one 256 B line per plane.
// Invalid pixels get NaN in all three planes (the reference writes x = NaN only; consumers test x only).
// ------------------------------------------------------------------------------------------------
// (vertex_from_depth: mf_frame_pyramid_device.h)
__global__ __launch_bounds__(256) void k_vmap_nmap(const float* __restrict__ depth, float* __restrict__ vmap,
                                                   float* __restrict__ nmap, int W, int H, Intr k, float cutoff) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u >= W || v >= H) return;
    const int P = W * H, i = v * W + u;
    const float fx_inv = 1.f / k.fx, fy_inv = 1.f / k.fy;
    float3 v00, v01, v10;
    const bool ok00 = vertex_from_depth(depth[i], u, v, k, fx_inv, fy_inv, cutoff, v00);
    vmap[i] = v00.x; vmap[P + i] = v00.y; vmap[2 * P + i] = v00.z;
    float3 n = f3(qnan(), qnan(), qnan());
    if (u < W - 1 && v < H - 1) {
        const bool ok01 = vertex_from_depth(depth[i + 1], u + 1, v, k, fx_inv, fy_inv, cutoff, v01);
        const bool ok10 = vertex_from_depth(depth[i + W], u, v + 1, k, fx_inv, fy_inv, cutoff, v10);
        if (ok00 && ok01 && ok10) n = normalized_rsqrt(cross3(v01 - v00, v10 - v00));
    }
    nmap[i] = n.x; nmap[P + i] = n.y; nmap[2 * P + i] = n.z;
}

void launch_vmap_nmap(const float* depth, float* vmap, float* nmap, int W, int H, Intr k, float cutoff, hipStream_t s) {
    dim3 grid((W + 63) / 64, (H + 3) / 4);
    hipLaunchKernelGGL(k_vmap_nmap, grid, dim3(256), 0, s, depth, vmap, nmap, W, H, k, cutoff);
}

// Model::generateCUDATextures in ONE launch: the body lives in mf_frame_pyramid_device.h (shared with the launch that runs it beside the
// model-side pyramid, mf_model_pyramid.hip: k_frame_model_pyramid)
__global__ __launch_bounds__(256) void k_frame_pyramid(const FramePyrArgs a) {
    __shared__ float lds[kFpLdsFloats];
    frame_pyramid_body(a, lds, (int)blockIdx.x);
}

void launch_frame_pyramid(const float* depth, float* const vmap[3], float* const nmap[3], int W, int H, Intr k, float cutoff,
                          hipStream_t s) {
    FramePyrArgs a;
    a.depth = depth; a.W = W; a.H = H; a.k = k; a.cutoff = cutoff;
    for (int i = 0; i < 3; ++i) { a.vmap[i] = vmap[i]; a.nmap[i] = nmap[i]; }
    hipLaunchKernelGGL(k_frame_pyramid, dim3(xcd_padded_grid(frame_pyramid_tiles(W, H))), dim3(256), 0, s, a);
}

}  // namespace mf
