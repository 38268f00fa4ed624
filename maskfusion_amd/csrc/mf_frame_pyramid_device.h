// mf_frame_pyramid_device.h -- Model::generateCUDATextures' workgroup body (pyrDownGaussF x2 + createVMap / createNMap x3 of the frame's filtered
// depth), shared by k_frame_pyramid (mf_preproc.hip) and the launch that runs it beside the model-side pyramid (mf_model_pyramid.hip:
// k_frame_model_pyramid).  Every float operation of these functions is rounded on its own -- the pragma sits inside each body, and the helpers
// they call carry it too: the including file may allow contraction (mf_model_pyramid.hip does), and the preprocessing feeds normals, which amplify a
// 1-ulp depth difference ~1000x.
#pragma once
#include "mf_device.h"

namespace mf {

// binomial row {1,4,6,4,1}; the 5x5 kernel of pyrDownGaussF (cudafuncs.cu:517-521) is its outer product
__device__ __forceinline__ float gauss5(int i) { return i == 2 ? 6.f : ((i == 1 || i == 3) ? 4.f : 1.f); }

// normalized_rsqrt (mf_device.h) with its operations pinned: a * (1 / sqrt(dot(a, a)))
__device__ __forceinline__ float3 normalized_rsqrt_exact(float3 a) {
#pragma clang fp contract(off)
    const float d = a.x * a.x + a.y * a.y + a.z * a.z;
    const float s = 1.0f / sqrtf(d);
    return f3(a.x * s, a.y * s, a.z * s);
}

__device__ __forceinline__ bool vertex_from_depth(float z, int u, int v, Intr k, float fx_inv, float fy_inv, float cutoff,
                                                  float3& out) {
#pragma clang fp contract(off)
    if (z > 0.0f && z < cutoff) {
        out = f3(z * ((float)u - k.cx) * fx_inv, z * ((float)v - k.cy) * fy_inv, z);
        return true;
    }
    out = f3(qnan(), qnan(), qnan());
    return false;
}

// ------------------------------------------------------------------------------------------------
// Model::generateCUDATextures in ONE launch (Core/Model/Model.cpp:350-389): pyrDownGaussF x2 + createVMap/createNMap x3.
// A 256-thread workgroup owns a 4x4 tile of level 2 = 8x8 of level 1 = 16x16 of level 0 (1200 workgroups at VGA; 8x8 tiles
// = 300 workgroups left the chip half empty: 17 us).  It stages the 29x29 level-0 depths those need (5x5 taps of 5x5 taps
// + the +1 neighbours of the normals), builds the 13x13 level-1 and 5x5 level-2 depths in LDS with exactly the per-pixel expressions of k_pyrdown_f (same loop bounds, same summation order: results are
// bit-identical to the level-by-level kernels), and writes the six planar maps.  Five dependent launches (2 x 7.8 us +
// 3 x 4.8 us: each one launch-latency bound) become one; the two smaller depth levels never visit HBM.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pyrdown_px(const float* __restrict__ src /*LDS*/, int ldw, int ox, int oy, int x, int y, int sw, int sh) {
#pragma clang fp contract(off)
    const int tx = min(2 * x + 3, sw - 1);
    const int ty = min(2 * y + 3, sh - 1);
    float sum = 0.f;
    int count = 0;
    if (2 * x >= 2 && 2 * y >= 2 && tx == 2 * x + 3 && ty == 2 * y + 3) {
        // away from the image border the loops below are the full 5 x 5 window with the binomial weights in their natural order: the same taps in
        // the same order, unrolled and without a branch per tap -- a NaN tap adds +0 to the sum (which is never -0: it starts at +0 and every
        // addend is a depth >= 0 times a weight) and 0 to the count, i.e. nothing, as when it is skipped
        const float* p = src + (2 * y - 2 - oy) * ldw + (2 * x - 2 - ox);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const float v = p[j * ldw + i];
                const float w = gauss5(4 - j) * gauss5(4 - i);     // compile-time constant
                const bool ok = !isnan(v);
                sum += ok ? v * w : 0.f;
                count += ok ? (int)w : 0;
            }
        }
        return sum / (float)count;
    }
    for (int cy = max(0, 2 * y - 2); cy < ty; ++cy) {
        for (int cx = max(0, 2 * x - 2); cx < tx; ++cx) {
            const float v = src[(cy - oy) * ldw + (cx - ox)];
            if (!isnan(v)) {
                const float w = gauss5(ty - cy - 1) * gauss5(tx - cx - 1);
                sum += v * w;
                count += (int)w;
            }
        }
    }
    return sum / (float)count;
}

__device__ __forceinline__ void vmap_nmap_px(const float* __restrict__ d /*LDS*/, int ldw, int ox, int oy, int u, int v, int W, int H,
                                             Intr k, float cutoff, float* __restrict__ vmap, float* __restrict__ nmap) {
#pragma clang fp contract(off)
    const int P = W * H, i = v * W + u;
    const float fx_inv = 1.f / k.fx, fy_inv = 1.f / k.fy;
    const float* p = d + (v - oy) * ldw + (u - ox);
    float3 v00, v01, v10;
    const bool ok00 = vertex_from_depth(p[0], u, v, k, fx_inv, fy_inv, cutoff, v00);
    vmap[i] = v00.x; vmap[P + i] = v00.y; vmap[2 * P + i] = v00.z;
    float3 n = f3(qnan(), qnan(), qnan());
    if (u < W - 1 && v < H - 1) {
        const bool ok01 = vertex_from_depth(p[1], u + 1, v, k, fx_inv, fy_inv, cutoff, v01);
        const bool ok10 = vertex_from_depth(p[ldw], u, v + 1, k, fx_inv, fy_inv, cutoff, v10);
        if (ok00 && ok01 && ok10) n = normalized_rsqrt_exact(cross3_exact(v01 - v00, v10 - v00));
    }
    nmap[i] = n.x; nmap[P + i] = n.y; nmap[2 * P + i] = n.z;
}

struct FramePyrArgs {
    const float* depth; int W, H; Intr k; float cutoff;
    float* vmap[3]; float* nmap[3];
};

constexpr int kFpT2 = 4;                                   // level-2 tile side of a workgroup (16x16 level-0 pixels)
constexpr int kFpL2 = kFpT2 + 1, kFpL1 = 2 * kFpT2 + 5, kFpL0 = 2 * kFpL1 + 3;   // 5, 13, 29 with their halos
constexpr int kFpLdsFloats = kFpL0 * kFpL0 + kFpL1 * kFpL1 + kFpL2 * kFpL2;      // the three levels' depths of one tile

inline int frame_pyramid_tiles(int W, int H) { return (((W >> 2) + kFpT2 - 1) / kFpT2) * (((H >> 2) + kFpT2 - 1) / kFpT2); }

// lds: kFpLdsFloats floats; block: the workgroup's index in a grid of at least xcd_padded_grid(frame_pyramid_tiles(W, H)) workgroups of 256 threads;
// tid: the thread's index among the 256 that share the tile.
// kLeave: a workgroup without a tile leaves as a whole, before the first barrier (k_frame_pyramid, k_frame_model_pyramid).  false: it stays and takes
// part in the barriers only -- for a caller whose workgroup holds several tiles' worth of threads, each 256 with an LDS slice of their own
// (mf_splat.hip: k_splat_tile beside the tile pass), or threads that belong to no tile at all (enabled == false).  Every float operation is the same.
template <bool kLeave = true>
__device__ __forceinline__ void frame_pyramid_body(const FramePyrArgs& a, float* lds, const int block, const int tid = (int)threadIdx.x,
                                                   const bool enabled = true) {
#pragma clang fp contract(off)
    float* const s0 = lds;
    float* const s1 = s0 + kFpL0 * kFpL0;
    float* const s2 = s1 + kFpL1 * kFpL1;
    const int W0 = a.W, H0 = a.H, W1 = W0 >> 1, H1 = H0 >> 1, W2 = W0 >> 2, H2 = H0 >> 2;
    const int tiles_x = (W2 + kFpT2 - 1) / kFpT2, tiles = tiles_x * ((H2 + kFpT2 - 1) / kFpT2);
    const int tile = xcd_contiguous_tile(block, tiles);     // XCD k works on the k-th band of tile rows (mf_device.h)
    // (a block index beyond the padded grid would wrap into the next XCD's band: a caller that pads further has no tile there)
    const bool on = enabled && block < xcd_padded_grid(tiles) && tile < tiles;
    if (kLeave && !on) return;
    const int X2 = (tile % tiles_x) * kFpT2, Y2 = (tile / tiles_x) * kFpT2;  // tile origin at level 2
    const int ox1 = 2 * X2 - 2, oy1 = 2 * Y2 - 2;                // LDS origins (may be negative)
    const int ox0 = 2 * ox1 - 2, oy0 = 2 * oy1 - 2;
    if (on) for (int i = tid; i < kFpL0 * kFpL0; i += 256) {
        const int ly = i / kFpL0, lx = i - ly * kFpL0;
        const int gx = ox0 + lx, gy = oy0 + ly;
        s0[i] = (gx >= 0 && gx < W0 && gy >= 0 && gy < H0) ? a.depth[gy * W0 + gx] : qnan();
    }
    __syncthreads();
    // (each level's vertex / normal maps are written as soon as its depths stand in LDS: their stores drain under the next level's arithmetic)
    const Intr k0 = a.k;
    const Intr k1 = Intr{a.k.fx / 2.f, a.k.fy / 2.f, a.k.cx / 2.f, a.k.cy / 2.f};
    const Intr k2 = Intr{a.k.fx / 4.f, a.k.fy / 4.f, a.k.cx / 4.f, a.k.cy / 4.f};
    if (on) for (int l = tid; l < 16 * kFpT2 * kFpT2; l += 256) {
        const int u = 4 * X2 + l % (4 * kFpT2), v = 4 * Y2 + l / (4 * kFpT2);
        if (u < W0 && v < H0) vmap_nmap_px(s0, kFpL0, ox0, oy0, u, v, W0, H0, k0, a.cutoff, a.vmap[0], a.nmap[0]);
    }
    if (on) for (int i = tid; i < kFpL1 * kFpL1; i += 256) {
        const int ly = i / kFpL1, lx = i - ly * kFpL1;
        const int gx = ox1 + lx, gy = oy1 + ly;
        s1[i] = (gx >= 0 && gx < W1 && gy >= 0 && gy < H1) ? pyrdown_px(s0, kFpL0, ox0, oy0, gx, gy, W0, H0) : qnan();
    }
    __syncthreads();
    if (on) for (int l = tid; l < 4 * kFpT2 * kFpT2; l += 256) {
        const int u = 2 * X2 + l % (2 * kFpT2), v = 2 * Y2 + l / (2 * kFpT2);
        if (u < W1 && v < H1) vmap_nmap_px(s1, kFpL1, ox1, oy1, u, v, W1, H1, k1, a.cutoff, a.vmap[1], a.nmap[1]);
    }
    if (on) for (int i = tid; i < kFpL2 * kFpL2; i += 256) {
        const int ly = i / kFpL2, lx = i - ly * kFpL2;
        const int gx = X2 + lx, gy = Y2 + ly;
        s2[i] = (gx < W2 && gy < H2) ? pyrdown_px(s1, kFpL1, ox1, oy1, gx, gy, W1, H1) : qnan();
    }
    __syncthreads();
    if (on) for (int l = tid; l < kFpT2 * kFpT2; l += 256) {
        const int u = X2 + l % kFpT2, v = Y2 + l / kFpT2;
        if (u < W2 && v < H2) vmap_nmap_px(s2, kFpL2, X2, Y2, u, v, W2, H2, k2, a.cutoff, a.vmap[2], a.nmap[2]);
    }
}

}  // namespace mf
