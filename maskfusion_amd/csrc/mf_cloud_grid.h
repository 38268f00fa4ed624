// mf_cloud_grid.h -- the hashed uniform grid over a point cloud that mf_eval.hip builds (nn_build there) and every consumer walks: the
// grid's description, its cell arithmetic and the two walks (nn_walk_cells, nn_walk_records), which own the rounding argument.  Shared by
// mf_eval.hip (nearest neighbour, registration, normals, FPFH) and mf_mesh.hip (surfel meshing); the text below is the text mf_eval.hip
// held, moved here unchanged.  Both files are compiled with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#include "mf_internal.h"
#include "mf_device.h"

namespace mf {

constexpr int kNnThreads = 256;
constexpr int kNnScanBlocks = 1024;          // workgroups of the scan (slices of the bucket array)
constexpr int kNnMaxGrid = 65536;            // grid-stride launches: at most this many workgroups
constexpr unsigned kNnNoRank = 0xFFFFFFFFu;  // a target the grid does not hold (not finite)
constexpr double kNnCellLimit = 1073741824.0;   // |x / radius| < 2^30: cell coordinates fit an int with room for +-1

struct NnGrid {
    double inv_h, h;          // 1 / radius and radius, fp64
    double reach;             // radius (1 + 2^-20): bounds every |q - p| whose fp32 d2 passes the radius test (nn_cell_range)
    float r2;                 // fl(radius * radius): the test
    unsigned mask;            // B - 1
    float4* rec;              // [N] the targets in bucket order
    unsigned* start;          // [B + 1] bucket b: rec[start[b], start[b + 1])
    unsigned* rank;           // [N] slot of target j inside its bucket
    unsigned* sums;           // [kNnScanBlocks]
    int* flag;                // a coordinate out of range was met
};

__host__ __device__ __forceinline__ unsigned nn_hash(int x, int y, int z) {
    unsigned h = (unsigned)x * 0x8da6b343u ^ (unsigned)y * 0xd8163841u ^ (unsigned)z * 0xcb1ab31fu;
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ bool nn_finite(float x, float y, float z) { return x - x == 0.f && y - y == 0.f && z - z == 0.f; }   // (inf - inf, NaN: NaN)
__device__ __forceinline__ bool nn_in_range(const NnGrid& g, float x, float y, float z) {
    return fabs((double)x * g.inv_h) < kNnCellLimit && fabs((double)y * g.inv_h) < kNnCellLimit && fabs((double)z * g.inv_h) < kNnCellLimit;
}
__device__ __forceinline__ int nn_cell(const NnGrid& g, float x) { return (int)floor((double)x * g.inv_h); }

// ---------------- the walk over the grid: which cells a point has to visit ----------------
// The rounding argument, stated here once for every consumer of the grid (nn_find, the normals, both FPFH passes).
//   The bounds enclose the cell.  A target p passes the radius test of point x when fl(fl(x - p)^2 ...) <= fl(r^2), hence |x - p| <=
//   r (1 + 4 eps) < reach per axis; rounding is monotone and p is representable, so fl(x - reach) <= p <= fl(x + reach), and the cells of the
//   two bounds (nn_cell_range: the same fp64 product as nn_cell) enclose p's cell.
//   A cell beyond the gap can be skipped.  nn_box_gap is the squared distance from x to the cell's box, the box widened by 2^-20 of a cell
//   on each side for the fp64 rounding of the cell assignment, so every target the build put into the cell lies in the widened box; the
//   fp32 d2 of such a target is at least (1 - 2^-18) of the three axes' gaps added.  When that exceeds the limit -- what d2 may still be
//   of use: the radius test's r2, or the best d2 of a minimum so far -- no record of the cell can count.
// Two cells of one walk may share a bucket.  A minimum may meet a record twice; a sum must not, so nn_walk_records lets a record count only
// in the visit of its OWN cell (nn_cell of its coordinates, the build's product).
__device__ __forceinline__ void nn_cell_range(const NnGrid& g, float x, int& lo, int& hi) {
    lo = (int)floor(((double)x - g.reach) * g.inv_h);
    hi = (int)floor(((double)x + g.reach) * g.inv_h);
}
__device__ __forceinline__ double nn_box_gap(const NnGrid& g, double x, int c) {
    const double pad = g.h * 9.5367431640625e-07;
    const double lo = (double)c * g.h - pad, hi = (double)(c + 1) * g.h + pad;
    const double d = x < lo ? lo - x : (x > hi ? x - hi : 0.0);
    return d * d;
}
// cell(cx, cy, cz) for every cell of the ranges of (x, y, z), finite and in range, whose gap is not beyond limit() -- asked anew for every cell
template <class Limit, class Cell>
__device__ __forceinline__ void nn_walk_cells(const NnGrid& g, float x, float y, float z, Limit&& limit, Cell&& cell) {
    int x0, x1, y0, y1, z0, z1;
    nn_cell_range(g, x, x0, x1); nn_cell_range(g, y, y0, y1); nn_cell_range(g, z, z0, z1);
    for (int cz = z0; cz <= z1; ++cz) {
        const double gz = nn_box_gap(g, z, cz);
        for (int cy = y0; cy <= y1; ++cy) {
            const double gy = nn_box_gap(g, y, cy);
            for (int cx = x0; cx <= x1; ++cx) {
                const double gap = (gz + gy + nn_box_gap(g, x, cx)) * (1.0 - 3.814697265625e-06);
                if (gap > (double)limit()) continue;
                cell(cx, cy, cz);
            }
        }
    }
}
// f(record) for every record that passes mf_cloud_nn_dev's radius test for (x, y, z), each exactly once
template <class F>
__device__ __forceinline__ void nn_walk_records(const NnGrid& g, float x, float y, float z, F&& f) {
    nn_walk_cells(g, x, y, z, [&] { return g.r2; }, [&](int cx, int cy, int cz) {
        const unsigned b = nn_hash(cx, cy, cz) & g.mask;
        const unsigned e = g.start[b + 1];
        for (unsigned r = g.start[b]; r < e; ++r) {
            const float4 p = g.rec[r];
            const float fx = p.x - x, fy = p.y - y, fz = p.z - z;
            const float d2 = fx * fx + fy * fy + fz * fz;
            if (!(d2 <= g.r2)) continue;
            if (nn_cell(g, p.x) != cx || nn_cell(g, p.y) != cy || nn_cell(g, p.z) != cz) continue;   // another cell's record in a shared bucket
            f(p);
        }
    });
}

// ---------------- host side (mf_eval.hip) ----------------
// the grid of n_target targets and `radius` laid out in a workspace of nn_workspace_bytes(n_target) (mf_internal.h)
NnGrid nn_layout(void* d_ws, int64_t n_target, float radius);
// clears the flag and fills the grid (count, scan, scatter); normal_offset >= 0: the normals go to nrm by record slot
int nn_build(const NnGrid& g, const float* d_target, int target_stride, int normal_offset, float4* nrm, int64_t n_target, hipStream_t s,
             const char** why = nullptr);
// waits for the stream and reports the range flag
int nn_finish(const NnGrid& g, hipStream_t s, const char** why = nullptr);
// the grid's ordered scan on any array: the exclusive scan of d[0, n) in place, d[n] = the total; sums: kNnScanBlocks values of scratch
void nn_exclusive_scan(unsigned* d, unsigned* sums, unsigned n, hipStream_t s);

}  // namespace mf
