// mf_eval.hip -- run evaluation: fixed-radius nearest neighbour between two point clouds (mf_cloud_nn_dev, mf_model_cloud_nn_dev) and one
// Gauss-Newton step of a rigid registration on those correspondences (mf_cloud_icp_build_dev / mf_cloud_icp_step_dev, below).  No upstream
// twin: the reference writes its clouds (savePly) and poses (exportPoses) and leaves their evaluation to outside tools.
//
// Result (DESIGN.md "Cloud evaluation"): for query i, the target j with the smallest fp32 d2 = dx*dx + dy*dy + dz*dz (d = q - p, no
// contraction: this file is compiled with -ffp-contract=off) among the finite targets with d2 <= fl(radius * radius); ties go to the smallest j.
// dist[i] = sqrtf(d2), idx[i] = j, or +inf / -1 when there is none or the query is not finite.
//
// Shape: a hashed uniform grid of cell edge h = radius, built per call.
//   1. k_nn_count: one lane per target: its cell c = floor(x / h) per axis (in fp64: x * (1 / h)), bucket = hash(c) mod B (B a power of two >= 2 N),
//      rank = atomicAdd(count[bucket], 1).
//   2. k_nn_scan_sums + k_nn_scan_apply: the exclusive scan of the B counts in place (the ordered-compaction idiom of mf_surfel.hip: per-workgroup
//      slice sums, then every workgroup adds the sums before it).
//   3. k_nn_scatter: target j -> rec[start[bucket] + rank] = {x, y, z, j} (16 B; a bucket's records are contiguous, their order is the order of
//      the atomics -- the (d2, j) minimum does not depend on it).
//   4. k_nn_query: one lane per query: the cells that can hold a target within radius (fp64 bounds, see nn_cell_range), the query's own cell
//      first; a cell whose box lies farther than the best distance found so far is skipped.
// No bounding box is needed: two cells that share a bucket only cost time.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/maskfusion_amd.h"
#include "mf_internal.h"
#include "mf_device.h"
#include "mf_walk.h"

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

// The cells of one axis that can hold a target p the radius test accepts for query coordinate x.  The test passing means
// fl(fl(q - p)^2 ...) <= fl(r^2), hence |q - p| <= r (1 + 4 eps) < reach; rounding is monotone and p is representable, so
// fl(x - reach) <= p <= fl(x + reach) and the cells of the two bounds (the same fp64 product as nn_cell) enclose p's cell.
__device__ __forceinline__ void nn_cell_range(const NnGrid& g, float x, int& lo, int& hi) {
    lo = (int)floor(((double)x - g.reach) * g.inv_h);
    hi = (int)floor(((double)x + g.reach) * g.inv_h);
}
// Squared distance from x to the cell's box, lowered for the fp64 rounding of the cell assignment (2^-20 of a cell on each side).
__device__ __forceinline__ double nn_box_gap(const NnGrid& g, double x, int c) {
    const double pad = g.h * 9.5367431640625e-07;
    const double lo = (double)c * g.h - pad, hi = (double)(c + 1) * g.h + pad;
    const double d = x < lo ? lo - x : (x > hi ? x - hi : 0.0);
    return d * d;
}

// 1.  grid-stride over the targets
// (noff >= 0: the target carries a normal at p[noff .. noff + 2]; one that is not finite takes the target out like a position that is not)
__global__ __launch_bounds__(kNnThreads) void k_nn_count(const float* __restrict__ t, int stride, int noff, int n, NnGrid g) {
    for (int j = blockIdx.x * kNnThreads + threadIdx.x; j < n; j += gridDim.x * kNnThreads) {
        const float* p = t + (size_t)j * stride;
        const float x = p[0], y = p[1], z = p[2];
        unsigned r = kNnNoRank;
        if (nn_finite(x, y, z) && (noff < 0 || nn_finite(p[noff], p[noff + 1], p[noff + 2]))) {
            if (nn_in_range(g, x, y, z)) r = atomicAdd(&g.start[nn_hash(nn_cell(g, x), nn_cell(g, y), nn_cell(g, z)) & g.mask], 1u);
            else atomicOr(g.flag, 1);
        }
        g.rank[j] = r;
    }
}

// 2.  exclusive scan of start[0, B) in place, start[B] = the total.  Slices of whole 256-element steps, one per workgroup.
__device__ __forceinline__ unsigned nn_slice(unsigned n) {
    const unsigned c = (n + gridDim.x - 1) / gridDim.x;
    return ((c + kNnThreads - 1) / kNnThreads) * kNnThreads;
}
__device__ __forceinline__ unsigned nn_block_sum(unsigned v, unsigned* s_w) {
    v = (unsigned)wave_sum_i((int)v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned tot = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return tot;
}
__global__ __launch_bounds__(kNnThreads) void k_nn_scan_sums(NnGrid g, unsigned n) {
    __shared__ unsigned s_w[4];
    const unsigned slice = nn_slice(n), beg = blockIdx.x * slice, end = min(n, beg + slice);
    unsigned v = 0;
    for (unsigned i = beg + threadIdx.x; i < end; i += kNnThreads) v += g.start[i];
    const unsigned tot = nn_block_sum(v, s_w);
    if (threadIdx.x == 0) g.sums[blockIdx.x] = tot;
}
__global__ __launch_bounds__(kNnThreads) void k_nn_scan_apply(NnGrid g, unsigned n) {
    __shared__ unsigned s_w[4];
    unsigned v = 0;
    for (unsigned b = threadIdx.x; b < blockIdx.x; b += kNnThreads) v += g.sums[b];
    unsigned base = nn_block_sum(v, s_w);
    const unsigned slice = nn_slice(n), beg = blockIdx.x * slice, end = min(n, beg + slice);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned i0 = beg; i0 < end; i0 += kNnThreads) {
        const unsigned i = i0 + threadIdx.x;
        const unsigned c = i < end ? g.start[i] : 0u;
        const unsigned x = wave_scan(c, lane);
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        unsigned off = base;
        for (int w = 0; w < wave; ++w) off += s_w[w];
        const unsigned tot = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (i < end) g.start[i] = off + x - c;
        base += tot;
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) g.start[n] = base;
}

// 3.
__global__ __launch_bounds__(kNnThreads) void k_nn_scatter(const float* __restrict__ t, int stride, int noff, float4* __restrict__ nrm, int n, NnGrid g) {
    for (int j = blockIdx.x * kNnThreads + threadIdx.x; j < n; j += gridDim.x * kNnThreads) {
        const unsigned r = g.rank[j];
        if (r == kNnNoRank) continue;
        const float* p = t + (size_t)j * stride;
        const float x = p[0], y = p[1], z = p[2];
        const unsigned b = nn_hash(nn_cell(g, x), nn_cell(g, y), nn_cell(g, z)) & g.mask;
        const unsigned slot = g.start[b] + r;
        g.rec[slot] = make_float4(x, y, z, __int_as_float(j));
        if (noff >= 0) nrm[slot] = make_float4(p[noff], p[noff + 1], p[noff + 2], 0.f);   // (registration: the record's normal, same slot)
    }
}

// 4.
struct NnQuery {
    const float* q; int stride, n;
    int transform; float T[12];   // query -> target, row-major 3 x 4: x' = ((T0 x + T1 y) + T2 z) + T3
    float* dist; int* idx;
};
// (bk: the winner's slot in rec; the plain query does not use it)
__device__ __forceinline__ void nn_scan_bucket(const NnGrid& g, int cx, int cy, int cz, float x, float y, float z, float& bd2, int& bj, unsigned& bk) {
    const unsigned b = nn_hash(cx, cy, cz) & g.mask;
    const unsigned e = g.start[b + 1];
    for (unsigned k = g.start[b]; k < e; ++k) {
        const float4 p = g.rec[k];
        const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
        const float d2 = dx * dx + dy * dy + dz * dz;
        const int j = __float_as_int(p.w);
        if (d2 <= g.r2 && (d2 < bd2 || (d2 == bd2 && j < bj))) { bd2 = d2; bj = j; bk = k; }
    }
}
// query i in the target frame
__device__ __forceinline__ void nn_load_query(const float* __restrict__ q, int stride, int i, int transform, const float* T, float& x, float& y, float& z) {
    const float* qp = q + (size_t)i * stride;
    x = qp[0]; y = qp[1]; z = qp[2];
    if (transform) {
        const float tx = T[0] * x + T[1] * y + T[2] * z + T[3];
        const float ty = T[4] * x + T[5] * y + T[6] * z + T[7];
        const float tz = T[8] * x + T[9] * y + T[10] * z + T[11];
        x = tx; y = ty; z = tz;
    }
}
// The winner of query (x, y, z): bj = its index (-1: none), bd2 its fp32 d2, bk its slot in rec.  A query that is not finite has no winner; one
// out of the cell range raises the flag.
__device__ __forceinline__ void nn_find(const NnGrid& g, int n_target, float x, float y, float z, float& bd2, int& bj, unsigned& bk) {
    bd2 = INFINITY; bj = -1; bk = 0u;
    if (!nn_finite(x, y, z)) return;
    if (!nn_in_range(g, x, y, z)) { atomicOr(g.flag, 1); return; }
    if (n_target <= 0) return;
    const int ox = nn_cell(g, x), oy = nn_cell(g, y), oz = nn_cell(g, z);
    nn_scan_bucket(g, ox, oy, oz, x, y, z, bd2, bj, bk);
    int x0, x1, y0, y1, z0, z1;
    nn_cell_range(g, x, x0, x1); nn_cell_range(g, y, y0, y1); nn_cell_range(g, z, z0, z1);
    for (int cz = z0; cz <= z1; ++cz) {
        const double gz = nn_box_gap(g, z, cz);
        for (int cy = y0; cy <= y1; ++cy) {
            const double gy = nn_box_gap(g, y, cy);
            for (int cx = x0; cx <= x1; ++cx) {
                if (cx == ox && cy == oy && cz == oz) continue;
                // the fp32 d2 of any target in the cell is at least (1 - 2^-18) of the box gap: skip the cell when that exceeds
                // what can still win (the best d2 so far, or the radius test)
                const double gap = (gz + gy + nn_box_gap(g, x, cx)) * (1.0 - 3.814697265625e-06);
                if (gap > (double)(bj >= 0 ? bd2 : g.r2)) continue;
                nn_scan_bucket(g, cx, cy, cz, x, y, z, bd2, bj, bk);
            }
        }
    }
}
__global__ __launch_bounds__(kNnThreads) void k_nn_query(NnGrid g, NnQuery a, int n_target) {
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < a.n; i += gridDim.x * kNnThreads) {
        float x, y, z, bd2;
        int bj;
        unsigned bk;
        nn_load_query(a.q, a.stride, i, a.transform, a.T, x, y, z);
        nn_find(g, n_target, x, y, z, bd2, bj, bk);
        a.dist[i] = bj >= 0 ? sqrtf(bd2) : INFINITY;
        a.idx[i] = bj;
    }
}

// ---------------- one registration step (mf_cloud_icp_step_dev) ----------------
// Two launches.  k_icp_find is k_nn_query with another output: every query finds its winner by nn_find -- the correspondence set IS
// mf_cloud_nn_dev's -- and stores the winner's record slot (4 B).  k_icp_accum then streams over the queries and adds the rows of the Gauss-Newton
// system in fp64: point-to-plane r = n . (x' - p), J = [n, x' x n]; point-to-point the three rows of [I, -[x']x] with r = x' - p.  sys29
// (mf_k_gn_solve's layout): for i = 0..5: J_i J_i .. J_i J_5, J_i r; then sum r^2; then the number of correspondences.
// Why two: the walk is bound by the latency of its dependent loads and lives on occupancy (46 VGPRs); with the 29 fp64 accumulators in the same
// kernel it needs 118 VGPRs and halves the resident wavefronts.  The price is 8 B per query of slot traffic and the query read twice.
// Reduction, without a floating-point atomic: a lane sums its own queries in index order (the grid is a function of the query count alone),
// the wavefront adds its lanes by an xor butterfly, the four wavefronts meet in LDS and are added in order: one partial per workgroup.
// k_icp_sum then adds the partials in workgroup order.  Nothing depends on the order of execution.
constexpr int kIcpMaxBlocks = 4096;         // partials of a step (a 256-CU part holds 1024 workgroups of this kernel at 4 waves / SIMD)
constexpr int kIcpPartial = 32;             // doubles per partial (29 used)
struct IcpStep {
    const float* q; int stride, n;
    int transform; float T[12];
    const float4* nrm;                      // [N] normals by record slot (point-to-plane)
    double* partial;                        // [gridDim.x][kIcpPartial]
    unsigned* slot;                         // [n] the winner's record slot, kIcpNoSlot: none
};
constexpr unsigned kIcpNoSlot = 0xFFFFFFFFu;
__global__ __launch_bounds__(kNnThreads) void k_icp_find(NnGrid g, IcpStep a, int n_target) {
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < a.n; i += gridDim.x * kNnThreads) {
        float x, y, z, bd2;
        int bj;
        unsigned bk;
        nn_load_query(a.q, a.stride, i, a.transform, a.T, x, y, z);
        nn_find(g, n_target, x, y, z, bd2, bj, bk);
        a.slot[i] = bj >= 0 ? bk : kIcpNoSlot;
    }
}
__device__ __forceinline__ void icp_add_row(double (&s)[29], const double (&J)[6], double r) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) s[k++] += J[i] * J[j];
        s[k++] += J[i] * r;
    }
    s[27] += r * r;
}
template <bool PLANE>
__global__ __launch_bounds__(kNnThreads) void k_icp_accum(NnGrid g, IcpStep a) {
    __shared__ double s_p[kNnThreads / 64][29];
    double s[29];
#pragma unroll
    for (int k = 0; k < 29; ++k) s[k] = 0.0;
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < a.n; i += gridDim.x * kNnThreads) {
        const unsigned bk = a.slot[i];
        if (bk == kIcpNoSlot) continue;
        float x, y, z;
        nn_load_query(a.q, a.stride, i, a.transform, a.T, x, y, z);
        const float4 p = g.rec[bk];
        const double X = (double)x, Y = (double)y, Z = (double)z;
        const double dx = X - (double)p.x, dy = Y - (double)p.y, dz = Z - (double)p.z;
        if (PLANE) {
            const float4 nf = a.nrm[bk];
            const double nx = (double)nf.x, ny = (double)nf.y, nz = (double)nf.z;
            const double J[6] = {nx, ny, nz, Y * nz - Z * ny, Z * nx - X * nz, X * ny - Y * nx};
            icp_add_row(s, J, (nx * dx + ny * dy) + nz * dz);
        } else {
            const double J0[6] = {1.0, 0.0, 0.0, 0.0, Z, -Y};
            const double J1[6] = {0.0, 1.0, 0.0, -Z, 0.0, X};
            const double J2[6] = {0.0, 0.0, 1.0, Y, -X, 0.0};
            icp_add_row(s, J0, dx);
            icp_add_row(s, J1, dy);
            icp_add_row(s, J2, dz);
        }
        s[28] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < 29; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 29; ++k) s_p[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < 29) {
        double v = s_p[0][threadIdx.x];
        for (int w = 1; w < kNnThreads / 64; ++w) v += s_p[w][threadIdx.x];
        a.partial[(size_t)blockIdx.x * kIcpPartial + threadIdx.x] = v;
    }
}
__global__ __launch_bounds__(64) void k_icp_sum(const double* __restrict__ partial, int blocks, double* __restrict__ out29) {
    if (threadIdx.x >= 29) return;
    double v = 0.0;
    for (int b = 0; b < blocks; ++b) v += partial[(size_t)b * kIcpPartial + threadIdx.x];
    out29[threadIdx.x] = v;
}

// ---------------- live surfels of a model -> float4 points (mf_eval.inl) ----------------
// the live surfels in download order (mf_download_map: the runs in order, each run's first len slots) -> out, position + index; a surfel at or
// below the confidence threshold becomes a NaN point, which the grid does not hold
__global__ __launch_bounds__(kNnThreads) void k_nn_live_gather(Surfels s, const FrameDev* __restrict__ frame, const int* __restrict__ offs, float thr,
                                                               float4* __restrict__ out, int n) {
    for_each_live_ordered(s, frame, offs, n, [&](int from, int to) {
        const float4 p = s.pc[from];
        out[to] = p.w > thr ? make_float4(p.x, p.y, p.z, 0.f) : make_float4(NAN, NAN, NAN, 0.f);
    });
}
void launch_nn_gather(Surfels s, const FrameDev* frame, const int* offs, float thr, float4* out, int n, int max_runs, hipStream_t st) {
    const int blocks = std::max(1, std::min(max_runs, 2048));
    hipLaunchKernelGGL(k_nn_live_gather, dim3(blocks), dim3(kNnThreads), 0, st, s, frame, offs, thr, out, n);
}

// ---------------- host side ----------------
static uint64_t nn_buckets(int64_t n) {
    uint64_t b = 64;
    while (b < 2 * (uint64_t)n) b <<= 1;
    return b;
}
static uint64_t nn_align(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
// workspace: rec [N] float4 | start [B + 1] | rank [N] | sums [kNnScanBlocks] | flag
uint64_t nn_workspace_bytes(int64_t n_target) {
    const uint64_t n = (uint64_t)std::max<int64_t>(n_target, 0);
    return nn_align(n * 16) + nn_align((nn_buckets(n_target) + 1) * 4) + nn_align(n * 4) + nn_align(kNnScanBlocks * 4) + 256;
}
static int nn_grid_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kNnThreads - 1) / kNnThreads, kNnMaxGrid)); }

// the grid of n_target targets and `radius` laid out in a workspace of nn_workspace_bytes(n_target)
static NnGrid nn_layout(void* d_ws, int64_t n_target, float radius) {
    const uint64_t B = nn_buckets(n_target), N = (uint64_t)n_target;
    char* w = (char*)d_ws;
    NnGrid g;
    g.h = (double)radius; g.inv_h = 1.0 / (double)radius; g.reach = (double)radius * (1.0 + 9.5367431640625e-07);
    g.r2 = radius * radius; g.mask = (unsigned)(B - 1);
    g.rec = (float4*)w; w += nn_align(N * 16);
    g.start = (unsigned*)w; w += nn_align((B + 1) * 4);
    g.rank = (unsigned*)w; w += nn_align(N * 4);
    g.sums = (unsigned*)w; w += nn_align(kNnScanBlocks * 4);
    g.flag = (int*)w;
    return g;
}
// clears the flag and fills the grid (count, scan, scatter); normal_offset >= 0: the normals go to nrm by record slot
static int nn_build(const NnGrid& g, const float* d_target, int target_stride, int normal_offset, float4* nrm, int64_t n_target, hipStream_t s,
                    const char** why) {
    const uint64_t B = (uint64_t)g.mask + 1;
    if (hipMemsetAsync(g.start, 0, (B + 1) * 4, s) != hipSuccess || hipMemsetAsync(g.flag, 0, sizeof(int), s) != hipSuccess) { *why = "hipMemsetAsync failed"; return MF_EHIP; }
    if (n_target > 0) {
        const int nb = nn_grid_blocks(n_target);
        hipLaunchKernelGGL(k_nn_count, dim3(nb), dim3(kNnThreads), 0, s, d_target, target_stride, normal_offset, (int)n_target, g);
        hipLaunchKernelGGL(k_nn_scan_sums, dim3(kNnScanBlocks), dim3(kNnThreads), 0, s, g, (unsigned)B);
        hipLaunchKernelGGL(k_nn_scan_apply, dim3(kNnScanBlocks), dim3(kNnThreads), 0, s, g, (unsigned)B);
        hipLaunchKernelGGL(k_nn_scatter, dim3(nb), dim3(kNnThreads), 0, s, d_target, target_stride, normal_offset, nrm, (int)n_target, g);
    }
    return MF_OK;
}
// column-major 4 x 4 (host) -> row-major 3 x 4
static void nn_transform_rows(const float* T16, float* T12) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) T12[r * 4 + c] = T16[c * 4 + r];
}
static bool nn_transform_finite(const float* T16) {
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(T16[k])) return false;
    return true;
}
// waits for the stream and reports the range flag
static int nn_finish(const NnGrid& g, hipStream_t s, const char** why) {
    if (hipGetLastError() != hipSuccess) { *why = "kernel launch failed"; return MF_EHIP; }
    int flag = 0;
    if (hipMemcpyAsync(&flag, g.flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        *why = "HIP error during the nearest-neighbour kernels"; return MF_EHIP;
    }
    if (flag) { *why = "a coordinate has |x / radius| >= 2^30"; return MF_EINVAL; }
    return MF_OK;
}

int nn_run(const float* d_target, int target_stride, int64_t n_target, const float* d_query, int query_stride, int64_t n_query,
           const float* T16, float radius, float* d_dist, int32_t* d_idx, void* d_ws, uint64_t ws_bytes, hipStream_t s, const char** why) {
    *why = nullptr;
    if (!(std::isfinite(radius) && radius > 0.f)) { *why = "radius must be finite and > 0"; return MF_EINVAL; }
    if (target_stride < 3 || query_stride < 3) { *why = "strides must be >= 3 floats"; return MF_EINVAL; }
    if (n_target < 0 || n_query < 0 || n_target > (int64_t)1 << 30 || n_query > (int64_t)1 << 30) { *why = "point count out of range"; return MF_EINVAL; }
    if ((n_target > 0 && !d_target) || (n_query > 0 && (!d_query || !d_dist || !d_idx))) { *why = "null pointer"; return MF_EINVAL; }
    if (!d_ws || ((uintptr_t)d_ws & 15) != 0 || ws_bytes < nn_workspace_bytes(n_target)) { *why = "workspace missing, misaligned or too small"; return MF_EINVAL; }
    if (T16 && !nn_transform_finite(T16)) { *why = "transform is not finite"; return MF_EINVAL; }
    const NnGrid g = nn_layout(d_ws, n_target, radius);
    const int rc = nn_build(g, d_target, target_stride, -1, nullptr, n_target, s, why);
    if (rc != MF_OK) return rc;
    if (n_query > 0) {
        NnQuery a;
        memset(&a, 0, sizeof(a));
        a.q = d_query; a.stride = query_stride; a.n = (int)n_query; a.dist = d_dist; a.idx = d_idx;
        if (T16) { a.transform = 1; nn_transform_rows(T16, a.T); }
        hipLaunchKernelGGL(k_nn_query, dim3(nn_grid_blocks(n_query)), dim3(kNnThreads), 0, s, g, a, (int)n_target);
    }
    return nn_finish(g, s, why);
}

// ---------------- registration: workspace = header (256 B) | the grid's workspace | normals [N] float4 | partials | slots [n_query] ----------------
constexpr uint64_t kIcpMagic = 0x3150434946444d4dull;   // a workspace mf_cloud_icp_build_dev has filled
struct IcpHeader { uint64_t magic; int64_t n_target; float radius; int32_t plane; };
static int icp_blocks(int64_t n_query) { return (int)std::max<int64_t>(1, std::min<int64_t>((n_query + kNnThreads - 1) / kNnThreads, kIcpMaxBlocks)); }
static uint64_t icp_partials_at(int64_t n_target) { return 256 + nn_workspace_bytes(n_target) + nn_align((uint64_t)std::max<int64_t>(n_target, 0) * 16); }
static uint64_t icp_slots_at(int64_t n_target) { return icp_partials_at(n_target) + nn_align((uint64_t)kIcpMaxBlocks * kIcpPartial * 8); }
static uint64_t icp_workspace_bytes(int64_t n_target, int64_t n_query) {
    return icp_slots_at(n_target) + nn_align((uint64_t)std::max<int64_t>(n_query, 0) * 4);
}
static bool icp_ws_ok(const void* d_ws, uint64_t bytes, uint64_t need) { return d_ws && ((uintptr_t)d_ws & 15) == 0 && bytes >= need; }

static int icp_build(const float* d_target, int target_stride, int normal_offset, int64_t n_target, float radius, void* d_ws, uint64_t ws_bytes,
                     hipStream_t s) {
    const char* why = nullptr;
    if (!(std::isfinite(radius) && radius > 0.f)) return MF_EINVAL;
    if (target_stride < 3 || (normal_offset >= 0 && (normal_offset < 3 || normal_offset + 3 > target_stride))) return MF_EINVAL;
    if (n_target < 0 || n_target > (int64_t)1 << 30 || (n_target > 0 && !d_target)) return MF_EINVAL;
    if (!icp_ws_ok(d_ws, ws_bytes, icp_workspace_bytes(n_target, 0))) return MF_EINVAL;
    char* w = (char*)d_ws;
    // not a built workspace until the build has gone through
    if (hipMemsetAsync(w, 0, 256, s) != hipSuccess) return MF_EHIP;
    const NnGrid g = nn_layout(w + 256, n_target, radius);
    float4* nrm = (float4*)(w + 256 + nn_workspace_bytes(n_target));
    int rc = nn_build(g, d_target, target_stride, normal_offset < 0 ? -1 : normal_offset, nrm, n_target, s, &why);
    if (rc != MF_OK) return rc;
    rc = nn_finish(g, s, &why);
    if (rc != MF_OK) return rc;
    const IcpHeader h = {kIcpMagic, n_target, radius, normal_offset >= 0 ? 1 : 0};
    if (hipMemcpyAsync(w, &h, sizeof(h), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return MF_EHIP;
    return MF_OK;
}

static int icp_step(void* d_ws, uint64_t ws_bytes, const float* d_query, int query_stride, int64_t n_query, const float* T16, double* d_out29,
                    hipStream_t s) {
    const char* why = nullptr;
    if (query_stride < 3 || n_query < 0 || n_query > (int64_t)1 << 30 || (n_query > 0 && !d_query) || !d_out29) return MF_EINVAL;
    if (!icp_ws_ok(d_ws, ws_bytes, 256)) return MF_EINVAL;
    if (T16 && !nn_transform_finite(T16)) return MF_EINVAL;
    char* w = (char*)d_ws;
    IcpHeader h;
    if (hipMemcpyAsync(&h, w, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return MF_EHIP;
    if (h.magic != kIcpMagic || h.n_target < 0 || h.n_target > (int64_t)1 << 30 || !(std::isfinite(h.radius) && h.radius > 0.f)) return MF_EINVAL;
    if (ws_bytes < icp_workspace_bytes(h.n_target, n_query)) return MF_EINVAL;
    const NnGrid g = nn_layout(w + 256, h.n_target, h.radius);
    if (hipMemsetAsync(g.flag, 0, sizeof(int), s) != hipSuccess) return MF_EHIP;
    IcpStep a;
    memset(&a, 0, sizeof(a));
    a.q = d_query; a.stride = query_stride; a.n = (int)n_query;
    if (T16) { a.transform = 1; nn_transform_rows(T16, a.T); }
    a.nrm = (const float4*)(w + 256 + nn_workspace_bytes(h.n_target));
    a.partial = (double*)(w + icp_partials_at(h.n_target));
    a.slot = (unsigned*)(w + icp_slots_at(h.n_target));
    const int nb = icp_blocks(n_query);
    if (n_query > 0) hipLaunchKernelGGL(k_icp_find, dim3(nn_grid_blocks(n_query)), dim3(kNnThreads), 0, s, g, a, (int)h.n_target);
    if (h.plane) hipLaunchKernelGGL(k_icp_accum<true>, dim3(nb), dim3(kNnThreads), 0, s, g, a);
    else hipLaunchKernelGGL(k_icp_accum<false>, dim3(nb), dim3(kNnThreads), 0, s, g, a);
    hipLaunchKernelGGL(k_icp_sum, dim3(1), dim3(64), 0, s, (const double*)a.partial, nb, d_out29);
    return nn_finish(g, s, &why);
}

}  // namespace mf

using namespace mf;

extern "C" int mf_cloud_nn_workspace(int64_t n_target, uint64_t* bytes) {
    if (!bytes || n_target < 0 || n_target > (int64_t)1 << 30) return MF_EINVAL;
    *bytes = nn_workspace_bytes(n_target);
    return MF_OK;
}

extern "C" int mf_cloud_nn_dev(const float* d_target, int32_t target_stride, int64_t n_target, const float* d_query, int32_t query_stride, int64_t n_query,
                               const float* query_to_target16, float radius, float* d_dist, int32_t* d_idx, void* d_workspace, uint64_t workspace_bytes,
                               void* stream) {
    const char* why = nullptr;
    return nn_run(d_target, target_stride, n_target, d_query, query_stride, n_query, query_to_target16, radius, d_dist, d_idx, d_workspace,
                  workspace_bytes, (hipStream_t)stream, &why);
}

extern "C" int mf_cloud_icp_workspace(int64_t n_target, int64_t n_query, uint64_t* bytes) {
    if (!bytes || n_target < 0 || n_target > (int64_t)1 << 30 || n_query < 0 || n_query > (int64_t)1 << 30) return MF_EINVAL;
    *bytes = icp_workspace_bytes(n_target, n_query);
    return MF_OK;
}

extern "C" int mf_cloud_icp_build_dev(const float* d_target, int32_t target_stride, int32_t normal_offset, int64_t n_target, float radius,
                                      void* d_workspace, uint64_t workspace_bytes, void* stream) {
    return icp_build(d_target, target_stride, normal_offset, n_target, radius, d_workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int mf_cloud_icp_step_dev(void* d_workspace, uint64_t workspace_bytes, const float* d_query, int32_t query_stride, int64_t n_query,
                                     const float* query_to_target16, double* d_out29, void* stream) {
    return icp_step(d_workspace, workspace_bytes, d_query, query_stride, n_query, query_to_target16, d_out29, (hipStream_t)stream);
}
