// mf_eval_trimesh.hip -- scoring against a triangle mesh: the exact distance from every query point to the nearest triangle within a radius,
// and a deterministic area-uniform sampler of the mesh (mf_trimesh_build_dev / mf_trimesh_distance_dev / mf_trimesh_sample_plan_dev /
// mf_trimesh_sample_emit_dev / mf_trimesh_free; DESIGN.md "Mesh evaluation").  No upstream twin: the reference never scores a map.
//
// The definition (include/maskfusion_amd.h has it in full).  A triangle is ELIGIBLE when its indices are in range, its nine coordinates are
// finite with |x / cell| < 2^30 and the fp64 squared norm of (b - a) x (c - a) is > 0.  The distance is Ericson's closest point (Real-Time
// Collision Detection 5.1.5) in fp64 from the fp32 values, every operation rounded on its own (the file is compiled without contraction), in
// the book's order of tests: vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, face.  The result of a query is the minimum over
// (D2, t) of the eligible triangles with D2 <= radius^2: a function of the mesh and the query alone, whatever the cell and whichever
// structure found the triangle.
//
// Shape.  The cells are those of mf_cloud_grid.h (nn_cell with h = cell, nn_hash into a power-of-two bucket array), holding TRIANGLES: a
// triangle is listed in every cell its bounding box covers.
//   1. k_tri_prep: one lane per triangle: eligibility, the 48-byte record (a, b, c as float4; a.w holds the index, -1: not eligible), and per
//      covered cell one atomicAdd on the bucket's count.  A triangle whose box covers more than kTriWideCells cells is not walked by one
//      lane: it goes to the WIDE list (its slot an atomic's rank; the order never shows, the result being a minimum over (D2, t)).
//   2. nn_exclusive_scan of the counts; the host reads the number of (triangle, cell) pairs and of wide triangles -- the one wait in the
//      middle, as in mf_cloud_mesh_build_dev -- and allocates the pair list.  k_tri_scatter fills it with a per-bucket cursor.
//   3. k_tri_query, the hot path: one lane per query, as k_nn_query.  Its own cell first, then nn_walk_cells over nn_cell_range(q -+ reach),
//      a cell skipped when its widened box lies beyond min(best D2, radius^2); then the wide list, each triangle's bounding box tested
//      against the same limit first.  A triangle met twice (several cells hold it; two cells share a bucket) is harmless for a minimum.
//      The rounding argument is mf_cloud_grid.h's: the closest point c of a counting triangle has |q - c| <= radius (1 + 2^-50) < reach per
//      axis and lies in the triangle's box, so its cell is both inside the walk and one of the cells the build listed the triangle in; that
//      cell's widened box is no farther from q than c, so the gap test (shrunk by 2^-18) cannot skip it while D2 can still win or tie.
//   4. k_tri_units / nn_exclusive_scan / k_tri_emit: the sampler.  Integer units of area (1 / 256 sample) per triangle, their ordered scan,
//      and per sample a binary search of its unit in the scan.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "mf_trimesh.h"

namespace mf {

// 1.
__global__ __launch_bounds__(kNnThreads) void k_tri_prep(const float* __restrict__ v, int vstride, int nv, const int* __restrict__ tri, TriDev m) {
    unsigned long long pairs = 0, eligible = 0;
    for (int t = blockIdx.x * kNnThreads + threadIdx.x; t < m.nt; t += gridDim.x * kNnThreads) {
        const int ia = tri[(size_t)t * 3], ib = tri[(size_t)t * 3 + 1], ic = tri[(size_t)t * 3 + 2];
        float4 a = make_float4(0.f, 0.f, 0.f, __int_as_float(-1)), b = make_float4(0.f, 0.f, 0.f, 0.f), c = b;
        bool ok = ia >= 0 && ia < nv && ib >= 0 && ib < nv && ic >= 0 && ic < nv;
        if (ok) {
            const float* pa = v + (size_t)ia * vstride; const float* pb = v + (size_t)ib * vstride; const float* pc = v + (size_t)ic * vstride;
            a.x = pa[0]; a.y = pa[1]; a.z = pa[2]; b.x = pb[0]; b.y = pb[1]; b.z = pb[2]; c.x = pc[0]; c.y = pc[1]; c.z = pc[2];
            ok = tri_coord_ok(m.g, a.x) && tri_coord_ok(m.g, a.y) && tri_coord_ok(m.g, a.z) && tri_coord_ok(m.g, b.x) && tri_coord_ok(m.g, b.y) &&
                 tri_coord_ok(m.g, b.z) && tri_coord_ok(m.g, c.x) && tri_coord_ok(m.g, c.y) && tri_coord_ok(m.g, c.z);
            double nx, ny, nz;
            if (ok) ok = tri_cross(a, b, c, nx, ny, nz) > 0.0;
        }
        if (ok) {
            a.w = __int_as_float(t);
            ++eligible;
            int lo[3], hi[3];
            const long long n = tri_box_cells(m.g, a, b, c, lo, hi);
            if (n < 0) m.wide[atomicAdd(&m.counters[kTriWide], 1ull)] = (unsigned)t;
            else {
                pairs += (unsigned long long)n;
                for (int cz = lo[2]; cz <= hi[2]; ++cz)
                    for (int cy = lo[1]; cy <= hi[1]; ++cy)
                        for (int cx = lo[0]; cx <= hi[0]; ++cx) atomicAdd(&m.g.start[nn_hash(cx, cy, cz) & m.g.mask], 1u);
            }
        } else {
            a = make_float4(0.f, 0.f, 0.f, __int_as_float(-1)); b = make_float4(0.f, 0.f, 0.f, 0.f); c = b;
        }
        m.rec[(size_t)t * 3] = a; m.rec[(size_t)t * 3 + 1] = b; m.rec[(size_t)t * 3 + 2] = c;
    }
    if (pairs) atomicAdd(&m.counters[kTriPairs], pairs);
    if (eligible) atomicAdd(&m.counters[kTriEligible], eligible);
}
// 2.
__global__ __launch_bounds__(kNnThreads) void k_tri_scatter(TriDev m) {
    for (int t = blockIdx.x * kNnThreads + threadIdx.x; t < m.nt; t += gridDim.x * kNnThreads) {
        const float4 a = m.rec[(size_t)t * 3], b = m.rec[(size_t)t * 3 + 1], c = m.rec[(size_t)t * 3 + 2];
        if (__float_as_int(a.w) < 0) continue;
        int lo[3], hi[3];
        if (tri_box_cells(m.g, a, b, c, lo, hi) < 0) continue;
        for (int cz = lo[2]; cz <= hi[2]; ++cz)
            for (int cy = lo[1]; cy <= hi[1]; ++cy)
                for (int cx = lo[0]; cx <= hi[0]; ++cx) {
                    const unsigned bk = nn_hash(cx, cy, cz) & m.g.mask;
                    m.items[m.g.start[bk] + atomicAdd(&m.cursor[bk], 1u)] = (unsigned)t;
                }
    }
}

// 3.  The closest point of triangle (a, b, c) to p, Ericson 5.1.5 in the book's order; returns D2 = |p - closest|^2
__device__ __forceinline__ double tri_closest(const float4& A, const float4& B, const float4& C, double px, double py, double pz, double& qx, double& qy, double& qz) {
    const double ax = (double)A.x, ay = (double)A.y, az = (double)A.z, bx = (double)B.x, by = (double)B.y, bz = (double)B.z;
    const double cx = (double)C.x, cy = (double)C.y, cz = (double)C.z;
    const double abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    [&] {
        const double d1 = tri_dot(abx, aby, abz, px - ax, py - ay, pz - az), d2 = tri_dot(acx, acy, acz, px - ax, py - ay, pz - az);
        if (d1 <= 0.0 && d2 <= 0.0) { qx = ax; qy = ay; qz = az; return; }                                        // vertex A
        const double d3 = tri_dot(abx, aby, abz, px - bx, py - by, pz - bz), d4 = tri_dot(acx, acy, acz, px - bx, py - by, pz - bz);
        if (d3 >= 0.0 && d4 <= d3) { qx = bx; qy = by; qz = bz; return; }                                         // vertex B
        const double vc = d1 * d4 - d3 * d2;
        if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                                                                // edge AB
            const double v = d1 / (d1 - d3);
            qx = ax + v * abx; qy = ay + v * aby; qz = az + v * abz;
            return;
        }
        const double d5 = tri_dot(abx, aby, abz, px - cx, py - cy, pz - cz), d6 = tri_dot(acx, acy, acz, px - cx, py - cy, pz - cz);
        if (d6 >= 0.0 && d5 <= d6) { qx = cx; qy = cy; qz = cz; return; }                                         // vertex C
        const double vb = d5 * d2 - d1 * d6;
        if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                                                                // edge AC
            const double w = d2 / (d2 - d6);
            qx = ax + w * acx; qy = ay + w * acy; qz = az + w * acz;
            return;
        }
        const double va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6;
        if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {                                                              // edge BC
            const double w = e43 / (e43 + e56);
            qx = bx + w * (cx - bx); qy = by + w * (cy - by); qz = bz + w * (cz - bz);
            return;
        }
        const double den = 1.0 / ((va + vb) + vc), v = vb * den, w = vc * den;                                    // face
        qx = (ax + abx * v) + acx * w; qy = (ay + aby * v) + acy * w; qz = (az + abz * v) + acz * w;
    }();
    const double ex = px - qx, ey = py - qy, ez = pz - qz;
    return (ex * ex + ey * ey) + ez * ez;
}
struct TriBest { double d2, x, y, z; int t; };
__device__ __forceinline__ void tri_test(const TriDev& m, unsigned t, double px, double py, double pz, double r2, TriBest& best) {
    if ((int)t == best.t) return;
    const float4 a = m.rec[(size_t)t * 3], b = m.rec[(size_t)t * 3 + 1], c = m.rec[(size_t)t * 3 + 2];
    double qx, qy, qz;
    const double d2 = tri_closest(a, b, c, px, py, pz, qx, qy, qz);
    if (d2 <= r2 && (d2 < best.d2 || (d2 == best.d2 && (int)t < best.t))) { best.d2 = d2; best.t = (int)t; best.x = qx; best.y = qy; best.z = qz; }
}
__device__ __forceinline__ void tri_scan_bucket(const TriDev& m, int cx, int cy, int cz, double px, double py, double pz, double r2, TriBest& best) {
    const unsigned bk = nn_hash(cx, cy, cz) & m.g.mask;
    const unsigned e = m.g.start[bk + 1];
    for (unsigned k = m.g.start[bk]; k < e; ++k) tri_test(m, m.items[k], px, py, pz, r2, best);
}
// squared distance from x to [lo, hi]
__device__ __forceinline__ double tri_axis_gap(double x, double lo, double hi) {
    const double d = x < lo ? lo - x : (x > hi ? x - hi : 0.0);
    return d * d;
}
struct TriQuery {
    const float* q; int stride, n;
    int transform; float T[12];   // query -> mesh, row-major 3 x 4, as NnQuery's
    double r2;                    // (double)radius * (double)radius
    float* dist; int* tri; float* closest;
};
__global__ __launch_bounds__(kNnThreads) void k_tri_query(TriDev m, TriQuery a) {
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < a.n; i += gridDim.x * kNnThreads) {
        const float* qp = a.q + (size_t)i * a.stride;
        float x = qp[0], y = qp[1], z = qp[2];
        if (a.transform) {   // mf_cloud_nn_dev's transform, bit for bit
            const float tx = a.T[0] * x + a.T[1] * y + a.T[2] * z + a.T[3];
            const float ty = a.T[4] * x + a.T[5] * y + a.T[6] * z + a.T[7];
            const float tz = a.T[8] * x + a.T[9] * y + a.T[10] * z + a.T[11];
            x = tx; y = ty; z = tz;
        }
        TriBest best;
        best.d2 = INFINITY; best.t = -1; best.x = best.y = best.z = 0.0;
        if (nn_finite(x, y, z)) {
            if (!nn_in_range(m.g, x, y, z)) atomicOr(m.g.flag, 1);
            else if (m.nt > 0) {
                const double px = (double)x, py = (double)y, pz = (double)z;
                const int ox = nn_cell(m.g, x), oy = nn_cell(m.g, y), oz = nn_cell(m.g, z);
                tri_scan_bucket(m, ox, oy, oz, px, py, pz, a.r2, best);
                nn_walk_cells(m.g, x, y, z, [&] { return best.t >= 0 ? best.d2 : a.r2; }, [&](int cx, int cy, int cz) {
                    if (cx == ox && cy == oy && cz == oz) return;
                    tri_scan_bucket(m, cx, cy, cz, px, py, pz, a.r2, best);
                });
                for (unsigned k = 0; k < m.n_wide; ++k) {
                    const unsigned t = m.wide[k];
                    const float4 A = m.rec[(size_t)t * 3], B = m.rec[(size_t)t * 3 + 1], C = m.rec[(size_t)t * 3 + 2];
                    const double gap = ((tri_axis_gap(px, (double)fminf(A.x, fminf(B.x, C.x)), (double)fmaxf(A.x, fmaxf(B.x, C.x))) +
                                         tri_axis_gap(py, (double)fminf(A.y, fminf(B.y, C.y)), (double)fmaxf(A.y, fmaxf(B.y, C.y)))) +
                                        tri_axis_gap(pz, (double)fminf(A.z, fminf(B.z, C.z)), (double)fmaxf(A.z, fmaxf(B.z, C.z)))) * (1.0 - 3.814697265625e-06);
                    if (gap > (best.t >= 0 ? best.d2 : a.r2)) continue;
                    tri_test(m, t, px, py, pz, a.r2, best);
                }
            }
        }
        const bool hit = best.t >= 0;
        a.dist[i] = hit ? (float)sqrt(best.d2) : INFINITY;
        a.tri[i] = best.t;
        if (a.closest) {
            a.closest[(size_t)i * 3] = hit ? (float)best.x : NAN;
            a.closest[(size_t)i * 3 + 1] = hit ? (float)best.y : NAN;
            a.closest[(size_t)i * 3 + 2] = hit ? (float)best.z : NAN;
        }
    }
}

// 4.  the sampler: u_t = llrint(0.5 |cross| density 256) units of 1 / 256 sample
__global__ __launch_bounds__(kNnThreads) void k_tri_units(TriDev m, double density) {
    unsigned long long total = 0;
    for (int t = blockIdx.x * kNnThreads + threadIdx.x; t < m.nt; t += gridDim.x * kNnThreads) {
        const float4 a = m.rec[(size_t)t * 3];
        unsigned u = 0;
        if (__float_as_int(a.w) >= 0) {
            double nx, ny, nz;
            const double n2 = tri_cross(a, m.rec[(size_t)t * 3 + 1], m.rec[(size_t)t * 3 + 2], nx, ny, nz);
            const double units = 0.5 * sqrt(n2) * density * 256.0;
            if (units < kTriTwo32) { u = (unsigned)llrint(units); total += u; }
            else total += 1ull << 32;                        // (the plan refuses a total of 2^32 or more)
        }
        m.S[t] = u;
    }
    if (total) atomicAdd(&m.counters[kTriUnits], total);
}
struct TriSamples { unsigned n; float* p; float* nrm; int* tri; };
__global__ __launch_bounds__(kNnThreads) void k_tri_emit(TriDev m, TriSamples o) {
    for (unsigned k = blockIdx.x * kNnThreads + threadIdx.x; k < o.n; k += gridDim.x * kNnThreads) {
        const unsigned unit = 256u * k + 128u;
        unsigned lo = 0, hi = (unsigned)m.nt;                // S[lo] <= unit < S[hi]
        while (hi - lo > 1) {
            const unsigned mid = lo + (hi - lo) / 2;
            if (m.S[mid] <= unit) lo = mid; else hi = mid;
        }
        const float4 a = m.rec[(size_t)lo * 3], b = m.rec[(size_t)lo * 3 + 1], c = m.rec[(size_t)lo * 3 + 2];
        const double k1 = (double)(k + 1u);
        double r1 = k1 * 0.7548776662466927, r2 = k1 * 0.5698402909980532;
        r1 = r1 - floor(r1); r2 = r2 - floor(r2);
        if (r1 + r2 > 1.0) { r1 = 1.0 - r1; r2 = 1.0 - r2; }
        const double ax = (double)a.x, ay = (double)a.y, az = (double)a.z;
        o.p[(size_t)k * 3] = (float)((ax + r1 * ((double)b.x - ax)) + r2 * ((double)c.x - ax));
        o.p[(size_t)k * 3 + 1] = (float)((ay + r1 * ((double)b.y - ay)) + r2 * ((double)c.y - ay));
        o.p[(size_t)k * 3 + 2] = (float)((az + r1 * ((double)b.z - az)) + r2 * ((double)c.z - az));
        if (o.nrm) {
            double nx, ny, nz;
            const double len = sqrt(tri_cross(a, b, c, nx, ny, nz));
            o.nrm[(size_t)k * 3] = (float)(nx / len); o.nrm[(size_t)k * 3 + 1] = (float)(ny / len); o.nrm[(size_t)k * 3 + 2] = (float)(nz / len);
        }
        if (o.tri) o.tri[k] = (int)lo;
    }
}

}  // namespace mf

using namespace mf;

extern "C" void mf_trimesh_free(mf_trimesh* h) {
    if (!h) return;
    if (h->d_main) (void)hipFree(h->d_main);
    if (h->d_items) (void)hipFree(h->d_items);
    delete h;
}

extern "C" int mf_trimesh_build_dev(const float* d_vertices, int32_t vertex_stride, int64_t n_vertices, const int32_t* d_triangles, int64_t n_triangles,
                                    float cell, mf_trimesh** out, uint32_t* n_eligible, void* stream) {
    if (!out || !n_eligible) return tri_fail("null pointer", MF_EINVAL);
    if (n_vertices < 0 || n_vertices > (int64_t)1 << 30 || n_triangles < 0 || n_triangles > (int64_t)1 << 30)
        return tri_fail("vertex or triangle count out of range (0 .. 2^30)", MF_EINVAL);
    if ((n_vertices > 0 && !d_vertices) || (n_triangles > 0 && !d_triangles)) return tri_fail("null vertices or triangles", MF_EINVAL);
    if (vertex_stride < 3) return tri_fail("vertex_stride must be >= 3 floats", MF_EINVAL);
    if (!tri_positive(cell)) return tri_fail("cell must be finite and > 0", MF_EINVAL);
    *out = nullptr; *n_eligible = 0;
    mf_trimesh* h = new mf_trimesh();
    memset(&h->m, 0, sizeof(h->m));
    h->cell = cell;
    TriDev& m = h->m;
    m.g.h = (double)cell; m.g.inv_h = 1.0 / (double)cell;
    m.nt = (int)n_triangles;
    if (n_triangles == 0) { *out = h; return MF_OK; }       // nothing to hold: every query misses, and there is nothing to sample

    hipStream_t s = (hipStream_t)stream;
    auto done = [&](int code, const char* text) {
        if (code != MF_OK) { mf_trimesh_free(h); return tri_fail(text, code); }
        *out = h; *n_eligible = h->eligible;
        return (int)MF_OK;
    };
    uint64_t B = 64;
    while (B < 2 * (uint64_t)n_triangles) B <<= 1;
    const uint64_t nt = (uint64_t)n_triangles;
    // rec | start [B + 1] | cursor [B] | wide [nt] | S [nt + 1] | sums | counters, flag
    const uint64_t o_start = tri_align(nt * 48), o_cursor = o_start + tri_align((B + 1) * 4), o_wide = o_cursor + tri_align(B * 4),
                   o_S = o_wide + tri_align(nt * 4), o_sums = o_S + tri_align((nt + 1) * 4), o_cnt = o_sums + tri_align(kNnScanBlocks * 4), total = o_cnt + 256;
    if (hipMalloc(&h->d_main, total) != hipSuccess) return done(MF_ENOMEM, "hipMalloc of the triangle records failed");
    char* w = (char*)h->d_main;
    m.rec = (float4*)w; m.g.start = (unsigned*)(w + o_start); m.cursor = (unsigned*)(w + o_cursor); m.wide = (unsigned*)(w + o_wide);
    m.S = (unsigned*)(w + o_S); m.g.sums = (unsigned*)(w + o_sums); m.counters = (unsigned long long*)(w + o_cnt);
    m.g.flag = (int*)(w + o_cnt + kTriCounters * 8);
    m.g.mask = (unsigned)(B - 1);
    if (hipMemsetAsync(w + o_start, 0, o_wide - o_start, s) != hipSuccess || hipMemsetAsync(w + o_cnt, 0, 256, s) != hipSuccess)
        return done(MF_EHIP, "hipMemsetAsync failed");
    const int nb = tri_blocks(n_triangles, kTriMaxBlocks);
    hipLaunchKernelGGL(k_tri_prep, dim3(nb), dim3(kNnThreads), 0, s, d_vertices, (int)vertex_stride, (int)n_vertices, (const int*)d_triangles, m);
    nn_exclusive_scan(m.g.start, m.g.sums, (unsigned)B, s);
    if (hipGetLastError() != hipSuccess) return done(MF_EHIP, "kernel launch failed");
    tri_bounds_dev(m, s);                                    // the ray caster's box of the gridded triangles: it rides on the read-back below
    if (hipGetLastError() != hipSuccess) return done(MF_EHIP, "kernel launch failed");
    unsigned long long cnt[kTriBoundsAt / 8 + 3] = {0, 0, 0, 0};   // the counters, the flag, and the box's six keys
    if (hipMemcpyAsync(cnt, m.counters, sizeof(cnt), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return done(MF_EHIP, "HIP error during the build kernels");
    h->gridded = tri_bounds_read((const unsigned*)(cnt + kTriBoundsAt / 8), h->lo, h->hi);
    h->eligible = (uint32_t)cnt[kTriEligible];
    m.n_wide = (unsigned)cnt[kTriWide];
    if (cnt[kTriPairs] >= (1ull << 32)) return done(MF_ENOMEM, "more than 2^32 (triangle, cell) pairs: use a larger cell");
    if (cnt[kTriPairs] > 0) {
        if (hipMalloc(&h->d_items, cnt[kTriPairs] * 4) != hipSuccess) return done(MF_ENOMEM, "hipMalloc of the cell lists failed");
        m.items = (unsigned*)h->d_items;
        hipLaunchKernelGGL(k_tri_scatter, dim3(nb), dim3(kNnThreads), 0, s, m);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return done(MF_EHIP, "HIP error during the scatter kernel");
    }
    return done(MF_OK, nullptr);
}

extern "C" int mf_trimesh_distance_dev(const mf_trimesh* h, const float* d_query, int32_t query_stride, int64_t n_query, const float* query_to_mesh16,
                                       float radius, float* d_dist, int32_t* d_tri, float* d_closest, void* stream) {
    if (!h) return tri_fail("null handle", MF_EINVAL);
    if (n_query < 0 || n_query > (int64_t)1 << 30) return tri_fail("query count out of range (0 .. 2^30)", MF_EINVAL);
    if (n_query > 0 && (!d_query || !d_dist || !d_tri)) return tri_fail("null queries or outputs", MF_EINVAL);
    if (query_stride < 3) return tri_fail("query_stride must be >= 3 floats", MF_EINVAL);
    if (!tri_positive(radius)) return tri_fail("radius must be finite and > 0", MF_EINVAL);
    if (radius > 16.f * h->cell) return tri_fail("radius must be <= 16 cell", MF_EINVAL);
    if (query_to_mesh16)
        for (int k = 0; k < 16; ++k)
            if (!std::isfinite(query_to_mesh16[k])) return tri_fail("transform is not finite", MF_EINVAL);
    if (n_query == 0) return MF_OK;
    hipStream_t s = (hipStream_t)stream;
    TriDev m = h->m;
    m.g.reach = (double)radius * (1.0 + 9.5367431640625e-07);
    m.g.r2 = radius * radius;
    TriQuery a;
    memset(&a, 0, sizeof(a));
    a.q = d_query; a.stride = query_stride; a.n = (int)n_query; a.r2 = (double)radius * (double)radius;
    a.dist = d_dist; a.tri = d_tri; a.closest = d_closest;
    if (query_to_mesh16) {
        a.transform = 1;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) a.T[r * 4 + c] = query_to_mesh16[c * 4 + r];
    }
    int* own_flag = nullptr;
    if (!m.g.flag) {                                        // a mesh of no triangles holds no device memory: the range flag of this call
        if (hipMalloc((void**)&own_flag, 256) != hipSuccess) return tri_fail("hipMalloc failed", MF_ENOMEM);
        m.g.flag = own_flag;
    }
    int flag = 0, rc = MF_OK;
    if (hipMemsetAsync(m.g.flag, 0, sizeof(int), s) != hipSuccess) rc = MF_EHIP;
    if (rc == MF_OK) {
        hipLaunchKernelGGL(k_tri_query, dim3(tri_blocks(n_query, kNnMaxGrid)), dim3(kNnThreads), 0, s, m, a);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&flag, m.g.flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            rc = MF_EHIP;
    }
    if (own_flag) (void)hipFree(own_flag);
    if (rc != MF_OK) return tri_fail("HIP error during the query kernel", rc);
    if (flag) return tri_fail("a query has |x / cell| >= 2^30", MF_EINVAL);
    return MF_OK;
}

extern "C" int mf_trimesh_sample_plan_dev(mf_trimesh* h, float density, uint64_t* n_samples, void* stream) {
    if (!h || !n_samples) return tri_fail("null pointer", MF_EINVAL);
    if (!tri_positive(density)) return tri_fail("density must be finite and > 0", MF_EINVAL);
    *n_samples = 0;
    h->planned = false; h->n_samples = 0;
    if (h->m.nt == 0) { h->planned = true; return MF_OK; }
    hipStream_t s = (hipStream_t)stream;
    TriDev& m = h->m;
    unsigned long long total = 0;
    if (hipMemsetAsync(&m.counters[kTriUnits], 0, 8, s) != hipSuccess) return tri_fail("hipMemsetAsync failed", MF_EHIP);
    hipLaunchKernelGGL(k_tri_units, dim3(tri_blocks(m.nt, kTriMaxBlocks)), dim3(kNnThreads), 0, s, m, (double)density);
    nn_exclusive_scan(m.S, m.g.sums, (unsigned)m.nt, s);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&total, &m.counters[kTriUnits], 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return tri_fail("HIP error during the plan kernels", MF_EHIP);
    if (total >= (1ull << 32)) return tri_fail("area x density x 256 reaches 2^32: sample at a lower density", MF_EINVAL);
    h->planned = true; h->n_samples = total / 256;
    *n_samples = h->n_samples;
    return MF_OK;
}

extern "C" int mf_trimesh_sample_emit_dev(const mf_trimesh* h, float* d_points, float* d_normals, int32_t* d_tri, void* stream) {
    if (!h) return tri_fail("null handle", MF_EINVAL);
    if (!h->planned) return tri_fail("no plan: call mf_trimesh_sample_plan_dev first", MF_EINVAL);
    if (h->n_samples > 0 && !d_points) return tri_fail("null output", MF_EINVAL);
    if (h->n_samples == 0) return MF_OK;
    hipStream_t s = (hipStream_t)stream;
    TriSamples o = {(unsigned)h->n_samples, d_points, d_normals, d_tri};
    hipLaunchKernelGGL(k_tri_emit, dim3(tri_blocks((int64_t)h->n_samples, kNnMaxGrid)), dim3(kNnThreads), 0, s, h->m, o);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return tri_fail("HIP error during the emit kernel", MF_EHIP);
    return MF_OK;
}
