// mf_sprite_device.h -- the arithmetic of the sprite passes, once: the prediction (ModelProjection::combinedPredict, Core/Shaders/splat.vert +
// combo_splat.frag) and GlobalProjection (splat_models.vert + combo_splat_models.frag) draw every surfel as a screen-space disc, each in a scatter
// form (one global atomicMin per covered pixel: mf_surfel.hip, mf_segment.hip) and a tiled form (z-test in LDS: mf_splat.hip).  All four run the
// per-surfel set-up, the viewing ray and the per-pixel ray/disc test below, so their keys are the same bits by construction.
// Raster rule: a sprite of side s centred on (u, v) covers pixel (px, py) iff u - s/2 <= px + 0.5 < u + s/2; LESS on the corrected z; the key's
// low word breaks ties (lower surfel index / earlier model in the list, GL draw order).
// (Kernel code, like mf_walk.h.  The including files switch fp contraction off before their headers.)
#pragma once

#include "mf_device.h"
#include "mf_walk.h"

namespace mf {

struct SplatSetup { float3 h, nrm; float sqrRad, pn; int px0, px1, py0, py1; };

// splat.vert:40-105 for surfel i of the view; false if it draws nothing.  time: the view's tick; Ri, ti: its pose's inverse, read once by the caller.
__device__ __forceinline__ bool splat_setup(const SpriteView& s, int i, float time, const float* Ri, float3 ti, SplatSetup& o) {
    const Surfels& src = s.src;
    const Intr k = s.k;
    const int W = s.W, H = s.H;
    const float4 pc = src.pc[i];
    if (pc.w < s.confThreshold) return false;
    const float lastTime = src.ct[i].w;
    const float3 h = mul33(Ri, f3(pc.x, pc.y, pc.z)) + ti;
    if (h.z > s.maxDepth || h.z < 0 || time - lastTime > (float)s.timeDelta || lastTime > time) return false;  // splat.vert:58, splat_models.vert:57
    const float u = ((k.fx * h.x) / h.z) + k.cx, v = ((k.fy * h.y) / h.z) + k.cy;
    if (!(u >= 0.f && u <= (float)W && v >= 0.f && v <= (float)H)) return false;
    const float4 n4 = src.nr[i];
    const float3 nrm = normalize_gl(mul33(Ri, f3(n4.x, n4.y, n4.z)));
    const float rad = n4.w;
    const float3 x1 = normalize_gl(f3(nrm.y - nrm.z, -nrm.x, nrm.x)) * (rad * 1.41421356f);
    const float3 y1 = cross3(nrm, x1);
    float xs0 = INFINITY, xs1 = -INFINITY, ys0 = INFINITY, ys1 = -INFINITY;
    const float3 corners[4] = {h + x1, h + y1, h - y1, h - x1};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float pxq = ((k.fx * corners[q].x) / corners[q].z) + k.cx;
        const float pyq = ((k.fy * corners[q].y) / corners[q].z) + k.cy;
        xs0 = fminf(xs0, pxq); xs1 = fmaxf(xs1, pxq);
        ys0 = fminf(ys0, pyq); ys1 = fmaxf(ys1, pyq);
    }
    float size = fmaxf(0.f, fmaxf(fabsf(xs1 - xs0), fabsf(ys1 - ys0)));
    if (!(size > 0.f)) return false;
    // gl_PointSize is clamped to the implementation's point size range (OpenGL 3.3 core, 3.4 "Points"; NVIDIA: [1, 2047]): a sprite
    // smaller than a pixel -- a surfel seen from more than ~4x its creation distance -- still covers the pixel its centre falls into
    size = fminf(fmaxf(size, 1.0f), 64.0f);
    const float half = size * 0.5f;
    o.px0 = max(0, (int)ceilf(u - half - 0.5f)); o.px1 = min(W - 1, (int)ceilf(u + half - 0.5f) - 1);
    o.py0 = max(0, (int)ceilf(v - half - 0.5f)); o.py1 = min(H - 1, (int)ceilf(v + half - 0.5f) - 1);
    if (o.px0 > o.px1 || o.py0 > o.py1) return false;
    o.h = h; o.nrm = nrm; o.sqrRad = rad * rad; o.pn = dot3(h, nrm);
    return true;
}

// the viewing ray of pixel (px, py) (combo_splat.frag:40-42): per covered pixel in the scatter forms, once per tile pixel (into LDS) in the tiled ones
__device__ __forceinline__ float3 sprite_ray(int px, int py, Intr k) {
    const float fcx = (float)px + 0.5f, fcy = (float)py + 0.5f;
    return normalize_gl(f3((fcx - k.cx) / k.fx, (fcy - k.cy) / k.fy, 1.0f));
}

// The ray/disc test of a pixel (combo_splat.frag:44-54): does the ray l meet the surfel's disc in front of the camera, and at which depth.  An
// edge-on disc (dot(l, n) = 0) divides by zero: the point is at infinity or NaN and fails the radius test.
__device__ __forceinline__ bool sprite_covers(const SplatSetup& su, float3 l, float& z) {
    const float3 cp = l * (su.pn / dot3(l, su.nrm));
    const float3 diff = cp - su.h;
    if (!(dot3(diff, diff) <= su.sqrRad)) return false;
    if (!(cp.z > 0.f)) return false;
    z = cp.z;
    return true;
}
// key = z bits << 32 | low word: the surfel's index (the prediction) or global_payload() (GlobalProjection)
__device__ __forceinline__ unsigned long long sprite_key(float z, unsigned low) { return ((unsigned long long)__float_as_uint(z) << 32) | low; }

// The scatter form of both passes: per-surfel sprite loop, 64-bit atomicMin per covered pixel.  kIndexKey: the key's low word is the surfel's
// index, else `payload`.  kLanes neighbouring lanes share one surfel and split its sprite's pixels between them as a kLX x kLY block (1: the
// thread-per-surfel form).  The object models' launches use 4: a few thousand sprites of 4-10 px a side kept a handful of threads busy for ~36 us
// each (round 4 trace), the rest of the GPU idle; the keys are the same bits in any split (atomicMin is order independent).
// pretest: zmin_key_pretested (the object models' launches).
template <int kLanes, bool kIndexKey>
__device__ __forceinline__ void sprite_scatter_body(const SpriteView& s, unsigned payload, unsigned long long* __restrict__ keys, bool pretest) {
    const float time = (float)s.frame->tick;  // combinedPredict(time = tick, maxTime = tick)
    float Ri[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Ri[q] = s.pose->Ri[q];
    const float3 ti = f3(s.pose->ti[0], s.pose->ti[1], s.pose->ti[2]);
    constexpr int kLX = kLanes >= 2 ? 2 : 1, kLY = kLanes / kLX;
    const int sub = threadIdx.x % kLanes, sx = sub % kLX, sy = sub / kLX;
    for_each_surfel_slice<kLanes>(s.src, s.frame, nullptr, nullptr, [&](int i, bool live) {
        if (!live) return;
        SplatSetup su;
        if (!splat_setup(s, i, time, Ri, ti, su)) return;
        for (int py = su.py0 + sy; py <= su.py1; py += kLY)
            for (int px = su.px0 + sx; px <= su.px1; px += kLX) {
                float z;
                if (!sprite_covers(su, sprite_ray(px, py, s.k), z)) continue;
                const unsigned long long key = sprite_key(z, kIndexKey ? (unsigned)i : payload);
                if (pretest) zmin_key_pretested(&keys[py * s.W + px], key);
                else zmin_key(&keys[py * s.W + px], key);
            }
    });
}

}  // namespace mf
