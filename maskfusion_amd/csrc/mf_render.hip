// mf_render.hip -- headless rendering of the surfel maps from a virtual pinhole camera (Model::renderPointCloud, Core/Model/Model.cpp:287-346,
// as MainController::drawScene calls it, GUI/MainController.cpp:609-720).  The semantics are restated in DESIGN.md ("Rendering"): every
// surfel is the disc of radius nr.w around its position in the plane normal to nr.xyz (the quad + discard of the geometry shader), a pixel is
// covered when the ray through its centre meets the disc, the smaller camera z wins (ties: the surfel drawn first), and the colour follows
// the colour type of the model.  Points mode: a confident surfel covers the one pixel its centre projects into.
//
// Shape (the prediction's, mf_splat.hip): per render
//   1. k_render_cull: one wavefront per run of every drawn model -- the run's largest radius and whether it holds a surfel above the model's
//      threshold (the run table keeps neither), then its box grown by that radius against the frustum with near / far; the surviving runs go
//      to the render's own list.  A dense buffer without a table is listed in chunks of kRun slots.
//   2. k_render_bin: one workgroup per listed run, one thread per slot: vertex test, disc box from the four projected quad corners (the whole
//      image when a corner lies before the near plane), one entry per 16 x 16 tile the box meets.
//   3. k_render_tile: one workgroup per tile: the rays of its 256 pixels in LDS, the disc test of every listed entry with ds_min_u64 on
//      {depth bits, draw index}, then one write per pixel of the winner's colour, depth and model.  A tile whose list ran over its slice scans
//      every listed run instead (nothing is lost).
// Nothing here writes model state: the render is read-only.
#pragma clang fp contract(off)

#include "mf_internal.h"
#include "mf_device.h"

namespace mf {

constexpr int kRTile = 16;          // tiles of 16 x 16 pixels
constexpr int kRTileThreads = kRTile * kRTile;
constexpr int kRCullThreads = 256;  // four runs (wavefronts) per workgroup
constexpr int kRBinThreads = kRun;  // one thread per slot of a run

struct RenderSetup { float3 h, n; float pn, r2; int x0, x1, y0, y1; };

// model -> view of point p (M row-major 3x4)
__device__ __forceinline__ float3 render_xform(const float* M, float3 p) {
    return f3(M[0] * p.x + M[1] * p.y + M[2] * p.z + M[3], M[4] * p.x + M[5] * p.y + M[6] * p.z + M[7], M[8] * p.x + M[9] * p.y + M[10] * p.z + M[11]);
}
__device__ __forceinline__ float3 render_rot(const float* M, float3 p) {
    return f3(M[0] * p.x + M[1] * p.y + M[2] * p.z, M[4] * p.x + M[5] * p.y + M[6] * p.z, M[8] * p.x + M[9] * p.y + M[10] * p.z);
}
__device__ __forceinline__ int render_clampi(float f, int lo, int hi) {
    if (!(f == f)) return lo;
    return (int)fminf(fmaxf(f, (float)lo), (float)hi);
}

// The vertex + geometry stage for slot i of model md: false if it draws nothing.  o: the disc in view coordinates and its pixel box.
__device__ __forceinline__ bool render_setup(const RenderArgs& a, const RenderModel& md, int i, RenderSetup& o) {
    const float4 pc = md.s.pc[i];
    const bool confident = pc.w > md.thr;
    const float4 n4 = md.s.nr[i];
    const float3 h = render_xform(md.M, f3(pc.x, pc.y, pc.z));
    if (a.drawPoints) {   // draw_feedback.vert: pc.w > threshold, one pixel
        if (!confident || !(h.z >= a.near_z && h.z <= a.far_z)) return false;
        const float u = a.k.fx * h.x / h.z + a.k.cx, v = a.k.fy * h.y / h.z + a.k.cy;
        if (!(u >= 0.f && u < (float)a.W && v >= 0.f && v < (float)a.H)) return false;
        o.x0 = o.x1 = min((int)floorf(u), a.W - 1); o.y0 = o.y1 = min((int)floorf(v), a.H - 1);
        o.h = h; o.n = f3(0.f, 0.f, 0.f); o.pn = 0.f; o.r2 = 0.f;
        return true;
    }
    if (!(confident || a.drawUnstable)) return false;   // draw_global_surface.vert
    const float3 n = render_rot(md.M, f3(n4.x, n4.y, n4.z));
    // draw_global_surface.geom: the quad around the disc (model frame), here only for the box
    const float3 nm = f3(n4.x, n4.y, n4.z);
    const float3 ax = f3(nm.y - nm.z, -nm.x, nm.x);
    const float al = sqrtf(dot3(ax, ax));
    if (!(al > 0.f)) return false;                      // degenerate quad: nothing is rasterised
    const float3 x1 = ax * (n4.w * 1.41421356f / al);
    const float3 y1 = cross3(nm, x1);
    const float3 p = f3(pc.x, pc.y, pc.z);
    const float3 cq[4] = {render_xform(md.M, p + x1), render_xform(md.M, p + y1), render_xform(md.M, p - y1), render_xform(md.M, p - x1)};
    int behind = 0, beyond = 0;
    float u0 = INFINITY, u1 = -INFINITY, v0 = INFINITY, v1 = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        behind += cq[q].z < a.near_z ? 1 : 0;
        beyond += cq[q].z > a.far_z ? 1 : 0;
        const float u = a.k.fx * cq[q].x / cq[q].z + a.k.cx, v = a.k.fy * cq[q].y / cq[q].z + a.k.cy;
        u0 = fminf(u0, u); u1 = fmaxf(u1, u); v0 = fminf(v0, v); v1 = fmaxf(v1, v);
    }
    if (behind == 4 || beyond == 4) return false;       // the disc lies in the quad's hull: all of it is before near / beyond far
    if (behind > 0) { o.x0 = 0; o.x1 = a.W - 1; o.y0 = 0; o.y1 = a.H - 1; }
    else {   // centres i + 0.5 in [u0, u1], one pixel of margin against the rounding of the corners
        o.x0 = render_clampi(floorf(u0 - 0.5f) - 1.f, 0, a.W); o.x1 = render_clampi(floorf(u1 - 0.5f) + 1.f, -1, a.W - 1);
        o.y0 = render_clampi(floorf(v0 - 0.5f) - 1.f, 0, a.H); o.y1 = render_clampi(floorf(v1 - 0.5f) + 1.f, -1, a.H - 1);
        if (!(u0 == u0 && u1 == u1 && v0 == v0 && v1 == v1)) { o.x0 = 0; o.x1 = a.W - 1; o.y0 = 0; o.y1 = a.H - 1; }
    }
    if (o.x0 > o.x1 || o.y0 > o.y1) return false;
    o.h = h; o.n = n; o.pn = dot3(h, n); o.r2 = n4.w * n4.w;
    return true;
}

// the disc test of one pixel (ray l = {(x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1}): camera z of the hit, or -1 if the pixel is not covered
__device__ __forceinline__ float render_hit(const RenderArgs& a, const RenderSetup& su, float2 l) {
    const float dn = l.x * su.n.x + l.y * su.n.y + su.n.z;
    const float t = su.pn / dn;
    const float3 cp = f3(l.x * t, l.y * t, t);
    const float3 d = cp - su.h;
    if (!(dot3(d, d) <= su.r2)) return -1.f;
    if (!(t >= a.near_z && t <= a.far_z)) return -1.f;
    return t;
}

__device__ __forceinline__ int render_find_model(const unsigned* base, int n, unsigned d) {
    int lo = 0, hi = n - 1;   // the last model whose first draw index is <= d
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (base[mid] <= d) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// per model: the transform model -> view.  Background (index 0 of the list): world -> view.  Object: (world -> view) . bgPose . pose^-1
// (MainController.cpp:684-686 draws it with pose * model.getPose().inverse(); the GlobalProjection kernels place it with the same product).
__global__ void k_render_setup(RenderModel* models, int n, const PoseDev* __restrict__ bg, RenderView v) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    RenderModel& md = models[m];
    float A[12];
    if (md.is_background) {
        for (int q = 0; q < 12; ++q) A[q] = q % 4 == 3 ? 0.f : ((q / 4) == (q % 4) ? 1.f : 0.f);
    } else {
        const PoseDev* p = md.pose;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) A[r * 4 + c] = bg->R[r * 3] * p->Ri[c] + bg->R[r * 3 + 1] * p->Ri[3 + c] + bg->R[r * 3 + 2] * p->Ri[6 + c];
            A[r * 4 + 3] = bg->R[r * 3] * p->ti[0] + bg->R[r * 3 + 1] * p->ti[1] + bg->R[r * 3 + 2] * p->ti[2] + bg->t[r];
        }
    }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 4; ++c) {
            float s = v.Vi[r * 4] * A[c] + v.Vi[r * 4 + 1] * A[4 + c] + v.Vi[r * 4 + 2] * A[8 + c];
            if (c == 3) s += v.Vi[r * 4 + 3];
            md.M[r * 4 + c] = s;
        }
    }
}

// step 1.  grid: (runs / 4, models); one wavefront per run (or per chunk of kRun slots of a dense buffer without a table)
__global__ __launch_bounds__(kRCullThreads) void k_render_cull(const RenderArgs a) {
    const RenderModel& md = a.models[blockIdx.y];
    const int r = blockIdx.x * (kRCullThreads / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= md.max_runs) return;
    const int runs = md.frame->runs;
    int beg, len;
    if (runs > 0) {
        if (r >= runs) return;
        beg = run_start(md.s.box, r); len = run_len(md.s.box, r);
    } else {
        beg = r * kRun; len = min(kRun, md.frame->count - beg);
    }
    if (len <= 0) return;   // (wavefront-uniform from here on)
    float rmax = 0.f;
    int stable = 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = lane; i < len; i += 64) {
        const float4 pc = md.s.pc[beg + i];
        rmax = fmaxf(rmax, fabsf(md.s.nr[beg + i].w));
        stable |= pc.w > md.thr ? 1 : 0;
        if (runs == 0) { lo[0] = fminf(lo[0], pc.x); lo[1] = fminf(lo[1], pc.y); lo[2] = fminf(lo[2], pc.z); hi[0] = fmaxf(hi[0], pc.x); hi[1] = fmaxf(hi[1], pc.y); hi[2] = fmaxf(hi[2], pc.z); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        rmax = fmaxf(rmax, __shfl_xor(rmax, o, 64));
        stable |= __shfl_xor(stable, o, 64);
        if (runs == 0)
            for (int q = 0; q < 3; ++q) { lo[q] = fminf(lo[q], __shfl_xor(lo[q], o, 64)); hi[q] = fmaxf(hi[q], __shfl_xor(hi[q], o, 64)); }
    }
    if (lane != 0) return;
    if (!stable && (a.drawPoints || !a.drawUnstable)) return;   // no surfel of the run passes the vertex test
    if (runs > 0) {
        const int4 bl = md.s.box[kBoxStride * r], bh = md.s.box[kBoxStride * r + 1];
        lo[0] = box_dec(bl.x); lo[1] = box_dec(bl.y); lo[2] = box_dec(bl.z); hi[0] = box_dec(bh.x); hi[1] = box_dec(bh.y); hi[2] = box_dec(bh.z);
    }
    if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return;   // (NaN positions draw nothing either)
    // the box of the centres grown by the largest radius holds every disc; 1 cm and 2 px against rounding
    const float g = a.drawPoints ? 0.f : rmax * 1.41421356f;
    int out_near = 1, out_far = 1, out_l = 1, out_r = 1, out_t = 1, out_b = 1;
    for (int c = 0; c < 8; ++c) {
        const float3 p = f3((c & 1) ? hi[0] + g : lo[0] - g, (c & 2) ? hi[1] + g : lo[1] - g, (c & 4) ? hi[2] + g : lo[2] - g);
        const float3 h = render_xform(md.M, p);
        out_near &= h.z < a.near_z - 0.01f;
        out_far &= h.z > a.far_z + 0.01f;
        out_l &= a.k.fx * h.x + (a.k.cx + 2.f) * h.z < 0.f;
        out_r &= a.k.fx * h.x + (a.k.cx - (float)a.W - 2.f) * h.z > 0.f;
        out_t &= a.k.fy * h.y + (a.k.cy + 2.f) * h.z < 0.f;
        out_b &= a.k.fy * h.y + (a.k.cy - (float)a.H - 2.f) * h.z > 0.f;
    }
    if (out_near | out_far | out_l | out_r | out_t | out_b) return;
    const int slot = atomicAdd(a.work_count, 1);
    a.work[slot] = ((int)blockIdx.y << 24) | r;
}

__device__ __forceinline__ void render_item(const RenderArgs& a, int item, int& m, int& beg, int& len) {
    m = (int)((unsigned)item >> 24);
    const int r = item & 0xFFFFFF;
    const RenderModel& md = a.models[m];
    if (md.frame->runs > 0) { beg = run_start(md.s.box, r); len = run_len(md.s.box, r); }
    else { beg = r * kRun; len = min(kRun, md.frame->count - beg); }
}

// step 2.  One listed run per workgroup round, one thread per slot
__global__ __launch_bounds__(kRBinThreads) void k_render_bin(const RenderArgs a) {
    const int n = *a.work_count;
    for (int w = blockIdx.x; w < n; w += gridDim.x) {
        int m, beg, len;
        render_item(a, a.work[w], m, beg, len);
        if ((int)threadIdx.x >= len) continue;
        const RenderModel& md = a.models[m];
        const int i = beg + (int)threadIdx.x;
        RenderSetup su;
        if (!render_setup(a, md, i, su)) continue;
        const unsigned d = md.base + (unsigned)i;
        for (int ty = su.y0 / kRTile; ty <= su.y1 / kRTile; ++ty)
            for (int tx = su.x0 / kRTile; tx <= su.x1 / kRTile; ++tx) {
                const int t = ty * a.tilesX + tx;
                const int slot = atomicAdd(&a.tile_count[t], 1);
                if (slot >= a.tile_cap) { *a.overflow = 1; continue; }   // the tile scans the listed runs instead (k_render_tile)
                const int lx0 = max(su.x0 - tx * kRTile, 0), lx1 = min(su.x1 - tx * kRTile, kRTile - 1);
                const int ly0 = max(su.y0 - ty * kRTile, 0), ly1 = min(su.y1 - ty * kRTile, kRTile - 1);
                a.entries[(size_t)t * a.tile_cap + slot] = make_uint2(d, (unsigned)(lx0 | (lx1 << 4) | (ly0 << 8) | (ly1 << 12)));
            }
    }
}

__device__ __forceinline__ float render_chan(float c) { return floorf(fminf(fmaxf(c, 0.f), 1.f) * 255.f + 0.5f); }

// step 3.  One workgroup of 256 threads per 16 x 16 tile
__global__ __launch_bounds__(kRTileThreads) void k_render_tile(const RenderArgs a) {
    __shared__ unsigned long long s_key[kRTileThreads];
    __shared__ float2 s_ray[kRTileThreads];
    __shared__ unsigned s_base[kMaxRenderModels];
    const int tile = blockIdx.x;
    const int tx0 = (tile % a.tilesX) * kRTile, ty0 = (tile / a.tilesX) * kRTile;
    const int lx = threadIdx.x & (kRTile - 1), ly = threadIdx.x >> 4;
    s_key[threadIdx.x] = kEmptyKey;
    s_ray[threadIdx.x] = make_float2(((float)(tx0 + lx) + 0.5f - a.k.cx) / a.k.fx, ((float)(ty0 + ly) + 0.5f - a.k.cy) / a.k.fy);
    for (int m = threadIdx.x; m < a.n_models; m += kRTileThreads) s_base[m] = a.models[m].base;
    __syncthreads();
    const int cnt = a.tile_count[tile];
    auto test = [&](const RenderSetup& su, unsigned d, int x0, int x1, int y0, int y1) {
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) {
                const int lp = y * kRTile + x;
                const float z = a.drawPoints ? su.h.z : render_hit(a, su, s_ray[lp]);
                if (!(z >= 0.f)) continue;
                atomicMin(&s_key[lp], ((unsigned long long)__float_as_uint(z) << 32) | d);
            }
    };
    if (cnt <= a.tile_cap) {
        const uint2* __restrict__ list = a.entries + (size_t)tile * a.tile_cap;
        for (int e = threadIdx.x; e < cnt; e += kRTileThreads) {
            const uint2 en = list[e];
            const int m = render_find_model(s_base, a.n_models, en.x);
            const RenderModel& md = a.models[m];
            const int i = (int)(en.x - md.base);
            const float4 pc = md.s.pc[i];
            RenderSetup su;
            su.h = render_xform(md.M, f3(pc.x, pc.y, pc.z));
            if (!a.drawPoints) {
                const float4 n4 = md.s.nr[i];
                su.n = render_rot(md.M, f3(n4.x, n4.y, n4.z));
                su.pn = dot3(su.h, su.n); su.r2 = n4.w * n4.w;
            }
            test(su, en.x, en.y & 15, (en.y >> 4) & 15, (en.y >> 8) & 15, (en.y >> 12) & 15);
        }
    } else {   // the list ran over its slice: every listed run, boxes recomputed
        const int n = *a.work_count;
        for (int w = 0; w < n; ++w) {
            int m, beg, len;
            render_item(a, a.work[w], m, beg, len);
            const RenderModel& md = a.models[m];
            for (int s = threadIdx.x; s < len; s += kRTileThreads) {
                RenderSetup su;
                if (!render_setup(a, md, beg + s, su)) continue;
                const int x0 = max(su.x0 - tx0, 0), x1 = min(su.x1 - tx0, kRTile - 1), y0 = max(su.y0 - ty0, 0), y1 = min(su.y1 - ty0, kRTile - 1);
                if (x0 > x1 || y0 > y1) continue;
                test(su, md.base + (unsigned)(beg + s), x0, x1, y0, y1);
            }
        }
    }
    __syncthreads();
    const int px = tx0 + lx, py = ty0 + ly;
    if (px >= a.W || py >= a.H) return;
    const size_t p = (size_t)py * a.W + px;
    const unsigned long long key = s_key[threadIdx.x];
    if (key == kEmptyKey) {
        a.out_rgba[p] = a.clear;
        if (a.out_depth) a.out_depth[p] = 0.f;
        if (a.out_model) a.out_model[p] = -1;
        return;
    }
    const unsigned d = (unsigned)(key & 0xFFFFFFFFull);
    const int m = render_find_model(s_base, a.n_models, d);
    const RenderModel& md = a.models[m];
    const int i = (int)(d - md.base);
    const float4 pc = md.s.pc[i], ct = md.s.ct[i], n4 = md.s.nr[i];
    const float time = (float)a.tick_frame->tick;
    const int ci = (int)ct.x;
    const float3 dec = f3((float)((ci >> 16) & 0xFF) / 255.0f, (float)((ci >> 8) & 0xFF) / 255.0f, (float)(ci & 0xFF) / 255.0f);
    const float dn = fabsf(n4.x + n4.y + n4.z);
    float3 c;
    if (a.drawPoints) {   // draw_feedback.vert
        c = md.color_type == 1 ? f3(n4.x, n4.y, n4.z) : md.color_type == 2 ? dec : f3(0.5f * dn + 0.1f, 0.5f * dn + 0.1f, 0.5f * dn + 0.1f);
    } else {              // draw_global_surface.geom
        if (md.color_type == 1) c = f3(n4.x, n4.y, n4.z);
        else if (md.color_type == 2) c = dec;
        else if (md.color_type == 3 || !(pc.w > md.thr)) {
            const float ratio = 2.f * (ct.z - 1.f) / (time - 1.f);
            const float r0 = fmaxf(0.f, 1.f - ratio), r1 = fmaxf(0.f, ratio - 1.f);
            const float s = dn + 0.1f;
            c = f3(r0 * s, r1 * s, (1.f - r0 - r1) * s);
        } else if (md.color_type == 4) {
            if (md.is_background) c = f3(0.5f * dn + 0.5f, 0.5f * dn + 0.5f, 0.5f * dn + 0.5f);
            else {
                const int q = ((md.class_id % a.n_palette) + a.n_palette) % a.n_palette;
                const float s = fmaxf(dn, 0.8f);
                c = f3(a.palette[3 * q] * s, a.palette[3 * q + 1] * s, a.palette[3 * q + 2] * s);
            }
        } else c = f3(0.5f * dn + 0.1f, 0.5f * dn + 0.1f, 0.5f * dn + 0.1f);
        if (a.drawWindow && time - ct.w > (float)a.timeDelta) c = c * 0.25f;
    }
    a.out_rgba[p] = make_uchar4((unsigned char)render_chan(c.x), (unsigned char)render_chan(c.y), (unsigned char)render_chan(c.z), 255);
    if (a.out_depth) a.out_depth[p] = __uint_as_float((unsigned)(key >> 32));
    if (a.out_model) a.out_model[p] = md.index;
}

void launch_render(RenderArgs a, const RenderView& v, const PoseDev* bg_pose, int max_runs, hipStream_t s) {
    if (a.n_models > 0) {   // (no model drawn: the tile pass only clears)
    hipLaunchKernelGGL(k_render_setup, dim3((a.n_models + 63) / 64), dim3(64), 0, s, a.models, a.n_models, bg_pose, v);
    hipLaunchKernelGGL(k_render_cull, dim3((max_runs + kRCullThreads / 64 - 1) / (kRCullThreads / 64), a.n_models), dim3(kRCullThreads), 0, s, a);
    hipLaunchKernelGGL(k_render_bin, dim3(2048), dim3(kRBinThreads), 0, s, a);
    }
    hipLaunchKernelGGL(k_render_tile, dim3(a.tilesX * a.tilesY), dim3(kRTileThreads), 0, s, a);
}

}  // namespace mf
