// mf_model_pyramid_device.h -- the arithmetic of the model-side pyramid (copyMaps + resize x2 + transform x3), shared by model_pyramid_body
// (mf_model_pyramid.hip: k_model_pyramid, k_bilateral_model_pyramid, k_frame_model_pyramid) and the epilogue of the tile pass that builds the same three
// levels from the prediction it has just drawn (mf_splat.hip: k_splat_tile, "tilePyramid").  Every float operation of these functions is pinned: the
// pragma sits inside each body and the fused multiply-adds are written out, in the form mf_model_pyramid.hip -- which allows contraction -- compiled
// them to before they moved here (read off the gfx950 ISA of the three kernels: R a as fma(R2, az, fma(R0, ax, R1 * ay)), the squared length of an
// averaged normal as fma(z, z, fma(x, x, y * y))).  mf_splat.hip has contraction off; written out, both files run the same instructions.
#pragma once
#include "mf_device.h"

namespace mf {

struct MapPx { float3 v, n; bool vok, nok; };

// copyMapsKernel (cudafuncs.cu:286-305) of one texel of the prediction
__device__ __forceinline__ MapPx copy_maps_px(float4 v4, float4 n4) {
    MapPx r;
    if (!(v4.z == 0)) {
        r.v = f3(v4.x, v4.y, v4.z); r.n = f3(n4.x, n4.y, n4.z);
        r.vok = !isnan(r.v.x); r.nok = !isnan(r.n.x);
    } else {
        r.v = r.n = f3(qnan(), qnan(), qnan());
        r.vok = r.nok = false;
    }
    return r;
}

// R a with the fused multiply-adds written out.  Under "fast" contraction the back end decides per use WHICH product of
// (R0 ax + R1 ay) + R2 az keeps its own rounding -- by operand order after scheduling: moving the model-side pyramid's body into a function (round 6)
// turned the level-2 normals' R1 ay into R0 ax and every fifth normal moved by an ulp, enough to shift a tracked pose by 1e-7 and flip a surfel of a
// count-exact test.  The form below is the one every use of the kernel compiled to through rounds 1-5; written out it no longer depends on context.
__device__ __forceinline__ float3 mul33_fixed(const float* R, float3 a) {
#pragma clang fp contract(off)
    return f3(fmaf(R[2], a.z, fmaf(R[0], a.x, R[1] * a.y)), fmaf(R[5], a.z, fmaf(R[3], a.x, R[4] * a.y)),
              fmaf(R[8], a.z, fmaf(R[6], a.x, R[7] * a.y)));
}

// normalized_rsqrt (mf_device.h) as the model-side pyramid's two uses compiled under contraction: the y product keeps its own rounding
__device__ __forceinline__ float3 normalized_rsqrt_fixed(float3 a) {
#pragma clang fp contract(off)
    const float d = fmaf(a.z, a.z, fmaf(a.x, a.x, a.y * a.y));
    const float s = 1.0f / sqrtf(d);
    return f3(a.x * s, a.y * s, a.z * s);
}

__device__ __forceinline__ void store_tx(float* __restrict__ vm, float* __restrict__ nm, int P, int i, float3 v, bool vok,
                                         float3 n, bool nok, const float* R, float3 t) {
#pragma clang fp contract(off)
    // tranformMapsKernel, cudafuncs.cu:207-249
    float3 vd = f3(qnan(), qnan(), qnan()), nd = vd;
    if (vok) vd = mul33_fixed(R, v) + t;
    if (nok) nd = mul33_fixed(R, n);
    vm[i] = vd.x; vm[P + i] = vd.y; vm[2 * P + i] = vd.z;
    nm[i] = nd.x; nm[P + i] = nd.y; nm[2 * P + i] = nd.z;
}

// value of lane (quad base + kB) for every lane of a quad: one DPP quad_perm broadcast, no LDS traffic
template <int kB>
__device__ __forceinline__ float quad_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kB | (kB << 2) | (kB << 4) | (kB << 6), 0xf, 0xf, false));
}
template <int kB>
__device__ __forceinline__ float3 quad_bcast3(float3 v) { return f3(quad_bcast<kB>(v.x), quad_bcast<kB>(v.y), quad_bcast<kB>(v.z)); }

// Levels 1 and 2 from the 2x2 level-0 texels of one level-1 texel (px, order x00 x01 x10 x11; read only where `inside`).  The four lanes of a DPP
// quad hold the 2x2 level-1 block of one level-2 texel in block order b = by * 2 + bx and exchange their values with quad broadcasts, so the
// averages keep the reference's operation order ((x00 + x01 + x10 + x11) / 4, level 2 from level-1 values; resizeMapKernel<false/true>,
// cudafuncs.cu:366-417).  Whole quads are inside or not; EVERY lane of the wavefront calls this (the broadcasts need the lanes in step).
// i1 / i2: the texel's index in the level-1 / level-2 planes of P1 / P2 texels.
__device__ __forceinline__ void model_pyramid_down(const MapPx* px, const bool inside, const int b, const float* R, const float3 t,
                                                   float* __restrict__ vm1, float* __restrict__ nm1, const int P1, const int i1,
                                                   float* __restrict__ vm2, float* __restrict__ nm2, const int P2, const int i2) {
#pragma clang fp contract(off)
    float3 v1 = f3(qnan(), qnan(), qnan()), n1 = v1;
    bool v1ok = false, n1ok = false;
    if (inside) {
        v1ok = px[0].vok && px[1].vok && px[2].vok && px[3].vok;
        n1ok = px[0].nok && px[1].nok && px[2].nok && px[3].nok;
        v1 = f3((px[0].v.x + px[1].v.x + px[2].v.x + px[3].v.x) / 4, (px[0].v.y + px[1].v.y + px[2].v.y + px[3].v.y) / 4,
                (px[0].v.z + px[1].v.z + px[2].v.z + px[3].v.z) / 4);
        n1 = normalized_rsqrt_fixed(f3((px[0].n.x + px[1].n.x + px[2].n.x + px[3].n.x) / 4,
                                       (px[0].n.y + px[1].n.y + px[2].n.y + px[3].n.y) / 4,
                                       (px[0].n.z + px[1].n.z + px[2].n.z + px[3].n.z) / 4));
        if (!v1ok) v1 = f3(qnan(), qnan(), qnan());
        if (!n1ok) n1 = f3(qnan(), qnan(), qnan());
        n1ok = n1ok && !isnan(n1.x);
        store_tx(vm1, nm1, P1, i1, v1, v1ok, n1, n1ok, R, t);
    }
    // level 2: the quad's four level-1 values in block order (executed by every lane: DPP needs them active)
    const float okv = v1ok ? 1.f : 0.f, okn = n1ok ? 1.f : 0.f;
    const float3 va = quad_bcast3<0>(v1), vb = quad_bcast3<1>(v1), vc = quad_bcast3<2>(v1), vd = quad_bcast3<3>(v1);
    const float3 na = quad_bcast3<0>(n1), nb = quad_bcast3<1>(n1), nc = quad_bcast3<2>(n1), nd = quad_bcast3<3>(n1);
    // (every broadcast is executed by every lane -- no short-circuit: the callers' wavefront reductions need the lanes in step)
    const float ov0 = quad_bcast<0>(okv), ov1 = quad_bcast<1>(okv), ov2 = quad_bcast<2>(okv), ov3 = quad_bcast<3>(okv);
    const float on0 = quad_bcast<0>(okn), on1 = quad_bcast<1>(okn), on2 = quad_bcast<2>(okn), on3 = quad_bcast<3>(okn);
    const bool v2ok = (ov0 != 0.f) & (ov1 != 0.f) & (ov2 != 0.f) & (ov3 != 0.f);
    bool n2ok = (on0 != 0.f) & (on1 != 0.f) & (on2 != 0.f) & (on3 != 0.f);
    if (inside && b == 0) {
        float3 v2 = f3((va.x + vb.x + vc.x + vd.x) / 4, (va.y + vb.y + vc.y + vd.y) / 4, (va.z + vb.z + vc.z + vd.z) / 4);
        float3 n2 = normalized_rsqrt_fixed(f3((na.x + nb.x + nc.x + nd.x) / 4, (na.y + nb.y + nc.y + nd.y) / 4, (na.z + nb.z + nc.z + nd.z) / 4));
        if (!v2ok) v2 = f3(qnan(), qnan(), qnan());
        if (!n2ok) n2 = f3(qnan(), qnan(), qnan());
        n2ok = n2ok && !isnan(n2.x);
        store_tx(vm2, nm2, P2, i2, v2, v2ok, n2, n2ok, R, t);
    }
}

}  // namespace mf
