// mf_trimesh.h -- the triangle-mesh handle (struct mf_trimesh), its device-side description (TriDev) and the small helpers that
// mf_eval_trimesh.hip (build, distance, sampler) and mf_trimesh_ray.hip (ray casting) share.  The text below is the text mf_eval_trimesh.hip
// held, moved here unchanged, plus the handle's bounding box of its gridded triangles, which the build fills for the ray caster.  Both
// files are compiled with -ffp-contract=off.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/maskfusion_amd.h"
#include "mf_internal.h"
#include "mf_device.h"
#include "mf_cloud_grid.h"

namespace mf {

constexpr long long kTriWideCells = 4096;      // a box of more cells than this: the wide list
constexpr int kTriMaxBlocks = 2048;            // workgroups of the per-triangle launches: a lane adds its counts up before its atomics
constexpr double kTriTwo32 = 4294967296.0;
enum { kTriPairs = 0, kTriEligible = 1, kTriWide = 2, kTriUnits = 3, kTriCounters = 4 };
// the handle's 256-byte block of counters: kTriCounters x 8 bytes, the range flag behind them, and at byte kTriBoundsAt six ordered keys --
// the bounding box of the gridded triangles (tri_bounds_dev)
constexpr int kTriBoundsAt = 64;

struct TriDev {
    NnGrid g;                      // h = cell, inv_h, mask, start [B + 1], sums, flag; reach and r2 are the query's
    int nt;                        // triangles of the caller's array
    float4* rec;                   // [nt][3] a, b, c; a.w: the index as bits, -1 when the triangle is not eligible
    unsigned* cursor;              // [B] the scatter's slots taken
    unsigned* items;               // [pairs] triangle indices in bucket order
    unsigned* wide;                // [nt] the wide triangles, n_wide of them
    unsigned n_wide;
    unsigned* S;                   // [nt + 1] the sampler's units: counts, then their exclusive scan
    unsigned long long* counters;  // [kTriCounters]
};

__device__ __forceinline__ bool tri_coord_ok(const NnGrid& g, float x) { return x - x == 0.f && fabs((double)x * g.inv_h) < kNnCellLimit; }
__device__ __forceinline__ double tri_dot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }
// |(b - a) x (c - a)|^2 in fp64, and the cross product itself
__device__ __forceinline__ double tri_cross(const float4& a, const float4& b, const float4& c, double& nx, double& ny, double& nz) {
    const double abx = (double)b.x - (double)a.x, aby = (double)b.y - (double)a.y, abz = (double)b.z - (double)a.z;
    const double acx = (double)c.x - (double)a.x, acy = (double)c.y - (double)a.y, acz = (double)c.z - (double)a.z;
    nx = aby * acz - abz * acy; ny = abz * acx - abx * acz; nz = abx * acy - aby * acx;
    return (nx * nx + ny * ny) + nz * nz;
}
// the cells of the triangle's bounding box; their number, or -1 when there are more than kTriWideCells
__device__ __forceinline__ long long tri_box_cells(const NnGrid& g, const float4& a, const float4& b, const float4& c, int (&lo)[3], int (&hi)[3]) {
    const float mn[3] = {fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z))};
    const float mx[3] = {fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z))};
    long long n = 1;
    for (int k = 0; k < 3; ++k) {
        lo[k] = nn_cell(g, mn[k]); hi[k] = nn_cell(g, mx[k]);
        const long long span = (long long)hi[k] - (long long)lo[k] + 1;
        if (span > kTriWideCells) return -1;
        n *= span;
    }
    return n > kTriWideCells ? -1 : n;
}

// enqueues the launch that folds the bounding box of the gridded (eligible, not wide) triangles of m.rec into the six keys at
// m.counters + kTriBoundsAt bytes, which must be zero (mf_trimesh_ray.hip); tri_bounds_read turns the keys, read back, into the box
void tri_bounds_dev(const TriDev& m, hipStream_t s);
bool tri_bounds_read(const unsigned* keys6, float* lo3, float* hi3);

}  // namespace mf

struct mf_trimesh {
    mf::TriDev m;
    float cell = 0.f;
    uint32_t eligible = 0;
    bool planned = false;
    uint64_t n_samples = 0;
    void* d_main = nullptr; void* d_items = nullptr;
    bool gridded = false;                     // some triangle is in the cells; then lo, hi: the fp32 bounding box of all such triangles
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
};

namespace mf {
static int tri_fail(const char* text, int rc) { return cloud_fail("mf_trimesh: ", text, rc); }
static int tri_blocks(int64_t n, int64_t cap) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kNnThreads - 1) / kNnThreads, cap)); }
static uint64_t tri_align(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
static bool tri_positive(float x) { return std::isfinite(x) && x > 0.f; }
}  // namespace mf
