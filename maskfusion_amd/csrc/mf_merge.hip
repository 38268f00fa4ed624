// mf_merge.hip -- map-to-map fusion (mf_cloud_merge_dev; DESIGN.md "Map merging"): every surfel of a source map, moved by a rigid transform,
// is merged into the surfel of a target map that stands for the same piece of surface, by the weighted rule of the frame fusion
// (Core/Shaders/update.vert:64-93), or appended when the target map has no such surfel.  No upstream twin: the reference fuses depth frames
// only, through the index map of one camera view (Model::fuse).  Fifth file of the evaluation family: it walks the hashed grid of
// mf_cloud_grid.h, which mf_eval.hip builds (nn_build), and needs no context.
//
// Shape (all on the caller's stream; one wait in the middle, for the count the capacity check needs, and one at the end):
//   1. nn_build of the targets with cell edge h = radius, the normals kept by record slot (what the registration does).
//   2. k_merge_find, a lane per source: transform, eligibility, then the walk of nn_find with one more test -- a record can only win when its
//      normal passes -- so the winner is the nearest target AMONG those that pass, not the nearest one tested afterwards.  Writes the partner
//      (or -1, -2), counts the sources of every target with an integer atomicAdd and flags the sources to append.
//   3. nn_exclusive_scan of the flags (a source's place behind the targets) and of the counts (where a target's list starts).
//      -- the host reads the range flag and the number to append; nothing has touched d_out so far --
//   4. k_merge_fill, a lane per matched source: list[start[j] + atomicAdd(cursor[j], 1)] = i.  The order inside a list is the order of the
//      atomics here, and it is put right in the next step.
//   5. k_merge_apply, a lane per target: sorts its list by insertion (quadratic in ONE list's length; a list is as long as the number of source
//      surfels on one target surfel, a handful when two maps of similar density meet), then copies its record and merges the sources in
//      ascending index, each into what the merge before it left.
//   6. k_merge_append, a lane per unmatched eligible source: its transformed record goes to d_out[n_target + scan].
// The only atomics are integer ones (counts, cursors, statistics) and nothing that reaches the output depends on their order: two calls give
// the same bytes.  The fp32 arithmetic is rounded operation by operation in the order the header gives (-ffp-contract=off, and the pragma for a
// build that forgets the flag).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/maskfusion_amd.h"
#include "mf_internal.h"
#include "mf_device.h"
#include "mf_cloud_grid.h"

namespace mf {

struct MergeRec { float4 p, c, n; };      // a record of mf_download_map: position + confidence | colour, unused, initTime, lastTime | normal + radius

struct MergeArgs {
    const float4* tgt; int nt;
    const float4* src; int ns;
    int transform; float T[12];             // source -> target, row-major 3 x 4
    float min_cos;
    const float4* nrm;                      // [nt] the targets' normals by record slot of the grid
    int* match;                             // [ns] partner, -1: none, -2: dropped
    unsigned* cnt;                          // [nt + 1] sources per target, after the scan: where the target's list starts
    unsigned* cursor;                       // [nt] zero on entry
    int* list;                              // [ns]
    unsigned* aflag;                        // [ns + 1] 1: to append; after the scan: its place behind the targets
    unsigned* stats;                        // [4] averaged, confidence-only, (unused: the scan's total is the appended count), dropped
    float4* out;
};

__device__ __forceinline__ bool merge_finite(float v) { return v - v == 0.f; }

// source i as the merge sees it; false: dropped
__device__ __forceinline__ bool merge_load_source(const MergeArgs& a, int i, MergeRec& r) {
    const float4* s = a.src + (size_t)i * 3;
    r.p = s[0]; r.c = s[1]; r.n = s[2];
    if (a.transform) {
        const float* T = a.T;
        const float x = r.p.x, y = r.p.y, z = r.p.z, nx = r.n.x, ny = r.n.y, nz = r.n.z;
        r.p.x = T[0] * x + T[1] * y + T[2] * z + T[3];
        r.p.y = T[4] * x + T[5] * y + T[6] * z + T[7];
        r.p.z = T[8] * x + T[9] * y + T[10] * z + T[11];
        r.n.x = T[0] * nx + T[1] * ny + T[2] * nz;
        r.n.y = T[4] * nx + T[5] * ny + T[6] * nz;
        r.n.z = T[8] * nx + T[9] * ny + T[10] * nz;
    }
    return nn_finite(r.p.x, r.p.y, r.p.z) && nn_finite(r.n.x, r.n.y, r.n.z) && merge_finite(r.p.w) && r.p.w > 0.f && merge_finite(r.n.w) && r.n.w > 0.f;
}

// nn_scan_bucket of mf_eval.hip with the normal test: a record that would win is asked for its normal, and wins only when it passes
__device__ __forceinline__ void merge_scan_bucket(const NnGrid& g, const MergeArgs& a, int cx, int cy, int cz, const MergeRec& s, float& bd2, int& bj) {
    const unsigned b = nn_hash(cx, cy, cz) & g.mask;
    const unsigned e = g.start[b + 1];
    for (unsigned k = g.start[b]; k < e; ++k) {
        const float4 p = g.rec[k];
        const float dx = s.p.x - p.x, dy = s.p.y - p.y, dz = s.p.z - p.z;
        const float d2 = dx * dx + dy * dy + dz * dz;
        const int j = __float_as_int(p.w);
        if (!(d2 <= g.r2 && (d2 < bd2 || (d2 == bd2 && j < bj)))) continue;
        const float4 q = a.nrm[k];
        if (!((s.n.x * q.x + s.n.y * q.y) + s.n.z * q.z >= a.min_cos)) continue;
        bd2 = d2; bj = j;
    }
}

__global__ __launch_bounds__(kNnThreads) void k_merge_find(NnGrid g, MergeArgs a) {
    unsigned dropped = 0;
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < a.ns; i += gridDim.x * kNnThreads) {
        MergeRec s;
        int bj = -1;
        if (!merge_load_source(a, i, s)) {
            bj = -2;
            ++dropped;
        } else if (!nn_in_range(g, s.p.x, s.p.y, s.p.z)) {
            atomicOr(g.flag, 1);
        } else if (a.nt > 0) {
            float bd2 = INFINITY;
            const int ox = nn_cell(g, s.p.x), oy = nn_cell(g, s.p.y), oz = nn_cell(g, s.p.z);
            merge_scan_bucket(g, a, ox, oy, oz, s, bd2, bj);
            // (as nn_find: the limit is what can still win, and a minimum may meet a record twice)
            nn_walk_cells(g, s.p.x, s.p.y, s.p.z, [&] { return bj >= 0 ? bd2 : g.r2; }, [&](int cx, int cy, int cz) {
                if (cx == ox && cy == oy && cz == oz) return;
                merge_scan_bucket(g, a, cx, cy, cz, s, bd2, bj);
            });
        }
        a.match[i] = bj;
        a.aflag[i] = bj == -1 ? 1u : 0u;
        if (bj >= 0) atomicAdd(&a.cnt[bj], 1u);
    }
    dropped = (unsigned)wave_sum_i((int)dropped);
    if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&a.stats[3], dropped);
}

__global__ __launch_bounds__(kNnThreads) void k_merge_fill(MergeArgs a) {
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < a.ns; i += gridDim.x * kNnThreads) {
        const int j = a.match[i];
        if (j >= 0) a.list[a.cnt[j] + atomicAdd(&a.cursor[j], 1u)] = i;
    }
}

// update.vert:64-93 with c = q's confidence and a = s's; returns true for the averaging branch
__device__ __forceinline__ bool merge_one(MergeRec& q, const MergeRec& s) {
    const float c = q.p.w, w = s.p.w, sum = c + w;
    const bool avg = s.n.w < 1.5f * q.n.w;
    if (avg) {
        q.p.x = (c * q.p.x + w * s.p.x) / sum;
        q.p.y = (c * q.p.y + w * s.p.y) / sum;
        q.p.z = (c * q.p.z + w * s.p.z) / sum;
        const float3 ok = decode_color(q.c.x), nk = decode_color(s.c.x);
        q.c.x = encode_color((c * ok.x + w * nk.x) / sum, (c * ok.y + w * nk.y) / sum, (c * ok.z + w * nk.z) / sum);
        const float3 n = f3((c * q.n.x + w * s.n.x) / sum, (c * q.n.y + w * s.n.y) / sum, (c * q.n.z + w * s.n.z) / sum);
        const float r = (c * q.n.w + w * s.n.w) / sum;
        const float3 u = normalized_rsqrt(n);
        q.n = make_float4(u.x, u.y, u.z, r);
    }
    q.p.w = sum;
    q.c.w = s.c.w > q.c.w ? s.c.w : q.c.w;
    return avg;
}

__global__ __launch_bounds__(kNnThreads) void k_merge_apply(MergeArgs a) {
    unsigned averaged = 0, conf_only = 0;
    for (int j = blockIdx.x * kNnThreads + threadIdx.x; j < a.nt; j += gridDim.x * kNnThreads) {
        const float4* t = a.tgt + (size_t)j * 3;
        MergeRec q = {t[0], t[1], t[2]};
        const unsigned b = a.cnt[j], e = a.cnt[j + 1];
        for (unsigned k = b + 1; k < e; ++k) {            // ascending source index: only this lane touches list[b, e)
            const int v = a.list[k];
            unsigned m = k;
            for (; m > b && a.list[m - 1] > v; --m) a.list[m] = a.list[m - 1];
            a.list[m] = v;
        }
        for (unsigned k = b; k < e; ++k) {
            MergeRec s;
            merge_load_source(a, a.list[k], s);
            if (merge_one(q, s)) ++averaged;
            else ++conf_only;
        }
        float4* o = a.out + (size_t)j * 3;
        o[0] = q.p; o[1] = q.c; o[2] = q.n;
    }
    averaged = (unsigned)wave_sum_i((int)averaged);
    conf_only = (unsigned)wave_sum_i((int)conf_only);
    if ((threadIdx.x & 63) == 0) {
        if (averaged) atomicAdd(&a.stats[0], averaged);
        if (conf_only) atomicAdd(&a.stats[1], conf_only);
    }
}

__global__ __launch_bounds__(kNnThreads) void k_merge_append(MergeArgs a) {
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < a.ns; i += gridDim.x * kNnThreads) {
        if (a.match[i] != -1) continue;
        MergeRec s;
        merge_load_source(a, i, s);
        float4* o = a.out + ((size_t)a.nt + a.aflag[i]) * 3;
        o[0] = s.p; o[1] = s.c; o[2] = s.n;
    }
}

// ---------------- host side ----------------
// workspace: the grid's | normals [nt] float4 | match [ns] | cnt [nt + 1] | cursor [nt] | list [ns] | aflag [ns + 1] | stats
static uint64_t merge_align(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
static bool merge_count_ok(int64_t n) { return n >= 0 && n <= (int64_t)1 << 30; }
static int merge_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kNnThreads - 1) / kNnThreads, kNnMaxGrid)); }
static uint64_t merge_workspace_bytes(int64_t n_target, int64_t n_source) {
    const uint64_t nt = (uint64_t)n_target, ns = (uint64_t)n_source;
    return nn_workspace_bytes(n_target) + merge_align(nt * 16) + merge_align(ns * 4) + merge_align((nt + 1) * 4) + merge_align(nt * 4) + merge_align(ns * 4) +
           merge_align((ns + 1) * 4) + 256;
}
static int merge_fail(const char* text, int rc) { return cloud_fail("mf_cloud_merge_dev: ", text, rc); }
static bool merge_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int merge_run(const float* d_target, int64_t n_target, const float* d_source, int64_t n_source, const float* T16, float radius, float min_cos,
                     float* d_out, int64_t out_capacity, int64_t* n_out, int32_t* d_match, uint64_t* stats4, void* d_ws, uint64_t ws_bytes, hipStream_t s) {
    if (!n_out || !stats4) return merge_fail("null pointer", MF_EINVAL);
    if (!(std::isfinite(radius) && radius > 0.f)) return merge_fail("radius must be finite and > 0", MF_EINVAL);
    if (!(min_cos >= -1.f && min_cos <= 1.f)) return merge_fail("min_cos must lie in [-1, 1]", MF_EINVAL);
    if (!merge_count_ok(n_target) || !merge_count_ok(n_source) || out_capacity < 0) return merge_fail("count out of range", MF_EINVAL);
    if ((n_target > 0 && !d_target) || (n_source > 0 && !d_source) || (out_capacity > 0 && !d_out)) return merge_fail("null pointer", MF_EINVAL);
    if (!merge_aligned(d_target) || !merge_aligned(d_source) || !merge_aligned(d_out)) return merge_fail("records must be 16-byte aligned", MF_EINVAL);
    if (!d_ws || !merge_aligned(d_ws) || ws_bytes < merge_workspace_bytes(n_target, n_source))
        return merge_fail("workspace missing, misaligned or too small", MF_EINVAL);
    if (T16)
        for (int k = 0; k < 16; ++k)
            if (!std::isfinite(T16[k])) return merge_fail("transform is not finite", MF_EINVAL);
    const uint64_t nt = (uint64_t)n_target, ns = (uint64_t)n_source;
    char* w = (char*)d_ws;
    const NnGrid g = nn_layout(w, n_target, radius);
    w += nn_workspace_bytes(n_target);
    MergeArgs a;
    memset(&a, 0, sizeof(a));
    a.tgt = (const float4*)d_target; a.nt = (int)n_target; a.src = (const float4*)d_source; a.ns = (int)n_source; a.min_cos = min_cos;
    a.out = (float4*)d_out;
    if (T16) {
        a.transform = 1;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) a.T[r * 4 + c] = T16[c * 4 + r];
    }
    float4* nrm = (float4*)w; a.nrm = nrm; w += merge_align(nt * 16);
    a.match = (int*)w; w += merge_align(ns * 4);
    a.cnt = (unsigned*)w; w += merge_align((nt + 1) * 4);
    a.cursor = (unsigned*)w; w += merge_align(nt * 4);
    a.list = (int*)w; w += merge_align(ns * 4);
    a.aflag = (unsigned*)w; w += merge_align((ns + 1) * 4);
    a.stats = (unsigned*)w;
    // cnt and cursor lie side by side: one memset
    if (hipMemsetAsync(a.cnt, 0, merge_align((nt + 1) * 4) + merge_align(nt * 4), s) != hipSuccess || hipMemsetAsync(a.aflag + ns, 0, 4, s) != hipSuccess ||
        hipMemsetAsync(a.stats, 0, 16, s) != hipSuccess)
        return merge_fail("hipMemsetAsync failed", MF_EHIP);
    const char* why = nullptr;
    int rc = nn_build(g, d_target, 12, 8, nrm, n_target, s, &why);
    if (rc != MF_OK) return merge_fail(why ? why : "grid build failed", rc);
    if (n_source > 0) {
        hipLaunchKernelGGL(k_merge_find, dim3(merge_blocks(n_source)), dim3(kNnThreads), 0, s, g, a);
        nn_exclusive_scan(a.aflag, g.sums, (unsigned)ns, s);
        if (n_target > 0) nn_exclusive_scan(a.cnt, g.sums, (unsigned)nt, s);
    }
    unsigned appended = 0;
    if (hipMemcpyAsync(&appended, a.aflag + ns, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return merge_fail("hipMemcpyAsync failed", MF_EHIP);
    rc = nn_finish(g, s, &why);                    // waits; a target or an eligible source out of the cell range
    if (rc != MF_OK) return merge_fail(why ? why : "HIP error", rc);
    *n_out = n_target + (int64_t)appended;
    if (out_capacity < *n_out) return merge_fail("out_capacity is smaller than the merged map (*n_out says how many records it has)", MF_ENOMEM);
    if (n_source > 0 && n_target > 0) hipLaunchKernelGGL(k_merge_fill, dim3(merge_blocks(n_source)), dim3(kNnThreads), 0, s, a);
    if (n_target > 0) hipLaunchKernelGGL(k_merge_apply, dim3(merge_blocks(n_target)), dim3(kNnThreads), 0, s, a);
    if (appended > 0) hipLaunchKernelGGL(k_merge_append, dim3(merge_blocks(n_source)), dim3(kNnThreads), 0, s, a);
    unsigned st[4] = {0, 0, 0, 0};
    if (hipGetLastError() != hipSuccess) return merge_fail("kernel launch failed", MF_EHIP);
    if (hipMemcpyAsync(st, a.stats, 16, hipMemcpyDeviceToHost, s) != hipSuccess ||
        (d_match && n_source > 0 && hipMemcpyAsync(d_match, a.match, ns * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        hipStreamSynchronize(s) != hipSuccess)
        return merge_fail("HIP error during the merge kernels", MF_EHIP);
    stats4[0] = st[0]; stats4[1] = st[1]; stats4[2] = appended; stats4[3] = st[3];
    return MF_OK;
}

}  // namespace mf

using namespace mf;

extern "C" int mf_cloud_merge_workspace(int64_t n_target, int64_t n_source, uint64_t* bytes) {
    if (!bytes || !merge_count_ok(n_target) || !merge_count_ok(n_source)) return MF_EINVAL;
    *bytes = merge_workspace_bytes(n_target, n_source);
    return MF_OK;
}

extern "C" int mf_cloud_merge_dev(const float* d_target, int64_t n_target, const float* d_source, int64_t n_source, const float* source_to_target16,
                                  float radius, float min_cos, float* d_out, int64_t out_capacity, int64_t* n_out, int32_t* d_match, uint64_t stats4[4],
                                  void* d_workspace, uint64_t workspace_bytes, void* stream) {
    return merge_run(d_target, n_target, d_source, n_source, source_to_target16, radius, min_cos, d_out, out_capacity, n_out, d_match, stats4,
                     d_workspace, workspace_bytes, (hipStream_t)stream);
}
