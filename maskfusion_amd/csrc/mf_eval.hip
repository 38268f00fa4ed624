// mf_eval.hip -- run evaluation on point clouds, all of it over one hashed grid: the fixed-radius nearest neighbour between two clouds
// (mf_cloud_nn_dev, mf_model_cloud_nn_dev), one Gauss-Newton step of a rigid registration on those correspondences (mf_cloud_icp_build_dev /
// mf_cloud_icp_step_dev), a cloud's normals (mf_cloud_normals_dev) and FPFH descriptors (mf_cloud_fpfh_dev), and the brute-force descriptor
// matcher (mf_feature_match_dev).  No upstream twin: the reference writes its clouds (savePly) and poses (exportPoses) and leaves their
// evaluation to outside tools.  The image scores of the evaluation are mf_eval_image.hip.
// Every consumer of the grid goes through the two walks of mf_cloud_grid.h (nn_walk_cells, nn_walk_records), which own the rounding argument.
//
// Nearest neighbour (DESIGN.md "Cloud evaluation"): for query i, the target j with the smallest fp32 d2 = dx*dx + dy*dy + dz*dz (d = q - p, no
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
#include "mf_cloud_grid.h"

namespace mf {


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
    // the limit of the walk: what can still win (the best d2 so far, or the radius test).  A minimum may meet a record twice: no own-cell test.
    nn_walk_cells(g, x, y, z, [&] { return bj >= 0 ? bd2 : g.r2; }, [&](int cx, int cy, int cz) {
        if (cx == ox && cy == oy && cz == oz) return;
        nn_scan_bucket(g, cx, cy, cz, x, y, z, bd2, bj, bk);
    });
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

// ---------------- normals of a cloud (mf_cloud_normals_dev; DESIGN.md "Cloud normals") ----------------
// The cloud is target and query at once.  Two launches over the grid nn_build makes of it.
// k_normals_walk: one lane per point i, grid-stride as k_nn_query.  nn_walk_records hands it every record j that passes mf_cloud_nn_dev's
// radius test (i itself does: d2 = 0), each once, and it adds d = p_j - p_i in fp64 to ten accumulators -- the count, sum d and the upper
// triangle of sum d d^T.  The nine sums go to a scratch record behind the grid (component-major, [9][n] doubles), the count to d_count.
// k_normals_solve: C = sum d d^T / k - m m^T, m = sum d / k, decomposed per lane by cyclic Jacobi rotations in fp64 (not the trigonometric
// closed form, which loses the small eigenvalue to cancellation), then the rules of the header.
// Why two, as k_icp_find / k_icp_accum: the walk lives on occupancy.  In one kernel the rotations' nine-double V and six-double C overlap the
// walk's registers only in part: 72 VGPRs, 7 wavefronts per SIMD.  Apart, the walk takes 64 -- the 8 wavefronts k_nn_query (47) has -- and
// the solve 62.  The price is 72 B per point written and read once.
// kNrmSweeps: Jacobi converges quadratically once the off-diagonal is small, and a 3 x 3 gets there in few sweeps; see DESIGN.md "Cloud
// normals" for how the count was chosen on the test clouds.
// A bucket's records lie in the order of the build's atomics, so the fp64 sums, and with them the normal, are reproducible to rounding
// only: the count is exact, the normal moves by about k 2^-53 over the relative eigenvalue gap from call to call.
constexpr int kNrmSweeps = 6;
struct NrmArgs {
    const float* p; int stride, n;
    int min_k;
    int has_view; float view[3];
    float4* out; int* count;
};
// rotation in the (p, q) plane that zeroes a_pq; r is the third index: (a_rp, a_rq) and the columns p, q of V turn with it
__device__ __forceinline__ void nrm_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double (&vp)[3], double (&vq)[3]) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // (theta^2 = inf: t = 0)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq; aqq += t * apq; apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq; arq = s * rp + c * rq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = vp[k], b = vq[k];
        vp[k] = c * a - s * b; vq[k] = s * a + c * b;
    }
}
// the ten sums of point (x, y, z), finite and in range: k and s = {sum d (3), the upper triangle of sum d d^T (6)}
__device__ __forceinline__ void nrm_walk(const NnGrid& g, float x, float y, float z, double (&s)[9], int& k) {
    nn_walk_records(g, x, y, z, [&](const float4& p) {
        const double dx = (double)p.x - (double)x, dy = (double)p.y - (double)y, dz = (double)p.z - (double)z;
        s[0] += dx; s[1] += dy; s[2] += dz;
        s[3] += dx * dx; s[4] += dx * dy; s[5] += dx * dz; s[6] += dy * dy; s[7] += dy * dz; s[8] += dz * dz;
        ++k;
    });
}
// sums -> (normal, surface variation), NaN where the rules give no normal
__device__ __forceinline__ float4 nrm_solve(const NrmArgs& a, float x, float y, float z, const double (&s)[9], int k) {
    const float4 none = make_float4(NAN, NAN, NAN, NAN);
    if (k < a.min_k) return none;
    const double ik = 1.0 / (double)k;
    const double mx = s[0] * ik, my = s[1] * ik, mz = s[2] * ik;
    double a00 = s[3] * ik - mx * mx, a01 = s[4] * ik - mx * my, a02 = s[5] * ik - mx * mz;
    double a11 = s[6] * ik - my * my, a12 = s[7] * ik - my * mz, a22 = s[8] * ik - mz * mz;
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};   // the columns of V
    for (int sweep = 0; sweep < kNrmSweeps; ++sweep) {
        nrm_rotate(a00, a11, a01, a02, a12, v0, v1);
        nrm_rotate(a00, a22, a02, a01, a12, v0, v2);
        nrm_rotate(a11, a22, a12, a01, a02, v1, v2);
    }
    // l0 <= l1 <= l2, n = the column of l0
    double l0 = a00, l1 = a11, l2 = a22, nx = v0[0], ny = v0[1], nz = v0[2];
    if (l1 < l0) { const double t = l0; l0 = l1; l1 = t; nx = v1[0]; ny = v1[1]; nz = v1[2]; }
    if (l2 < l0) { const double t = l0; l0 = l2; l2 = t; nx = v2[0]; ny = v2[1]; nz = v2[2]; }
    if (l2 < l1) { const double t = l1; l1 = l2; l2 = t; }
    if (l1 <= 1e-12 * l2) return none;
    const double inv = 1.0 / sqrt((nx * nx + ny * ny) + nz * nz);
    nx *= inv; ny *= inv; nz *= inv;
    // the sign: the viewpoint's side when there is one and it decides; else a rule of the vector alone (the component of largest magnitude
    // positive, ties to the lowest axis).  Nothing of the sweeps' history is left in it.
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    bool flip = ((ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz)) < 0.0;
    if (a.has_view) {
        const double dot = (nx * ((double)a.view[0] - (double)x) + ny * ((double)a.view[1] - (double)y)) + nz * ((double)a.view[2] - (double)z);
        if (dot != 0.0) flip = dot < 0.0;
    }
    if (flip) { nx = -nx; ny = -ny; nz = -nz; }
    return make_float4((float)nx, (float)ny, (float)nz, (float)(l0 / ((l0 + l1) + l2)));
}
__global__ __launch_bounds__(kNnThreads) void k_normals_walk(NnGrid g, NrmArgs a, double* __restrict__ sums) {
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < a.n; i += gridDim.x * kNnThreads) {
        const float* pp = a.p + (size_t)i * a.stride;
        const float x = pp[0], y = pp[1], z = pp[2];
        int k = 0;
        double s[9];
#pragma unroll
        for (int m = 0; m < 9; ++m) s[m] = 0.0;
        if (nn_finite(x, y, z)) {
            if (!nn_in_range(g, x, y, z)) atomicOr(g.flag, 1);
            else nrm_walk(g, x, y, z, s, k);
        }
#pragma unroll
        for (int m = 0; m < 9; ++m) sums[(size_t)m * a.n + i] = s[m];
        a.count[i] = k;
    }
}
__global__ __launch_bounds__(kNnThreads) void k_normals_solve(NrmArgs a, const double* __restrict__ sums) {
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < a.n; i += gridDim.x * kNnThreads) {
        const float* pp = a.p + (size_t)i * a.stride;
        double s[9];
#pragma unroll
        for (int m = 0; m < 9; ++m) s[m] = sums[(size_t)m * a.n + i];
        a.out[i] = nrm_solve(a, pp[0], pp[1], pp[2], s, a.count[i]);
    }
}

// ---------------- FPFH descriptors of a cloud (mf_cloud_fpfh_dev; DESIGN.md "Global registration") ----------------
// The cloud is target and query at once, as for the normals.  Four launches and the grid build between the first two:
// k_fpfh_prep: one lane per point: the eligible points (position and normal finite, the normal not zero) as float4 -- the others as NaN, which
//   the grid does not hold -- and the normals normalised in fp64, [n][4] doubles.  The grid is built of that copy, so a point that is not
//   eligible is nobody's neighbour and the grid code stays as it is.
// k_fpfh_spfh: one lane per point i, grid-stride as k_normals_walk.  Every record j != i that nn_walk_records hands over (the radius test, each
//   record once) gives one pair: its three bins from fpfh_pair, in fp64.  The 33 counters of a lane live in LDS, bin-major
//   (s_h[bin][lane]: a lane's column, no two lanes on one bank), because a histogram indexed by a computed bin cannot live in registers.
//   Integer counts: the SPFH does not depend on the order of a bucket's records.
// k_fpfh_sum: one wavefront per point, lane b < 33 owns bin b.  The wavefront walks the same cells in step (every lane tests the same
//   record: the loads are broadcasts), reads row j of the counts as one 136-byte line and lane b adds (1 / L^2) / k_j * SPFH_j[b] in fp64.
//   The three part sums are taken by 33 lane reads in bin order, the same for every lane, so a row is scaled by one value per part.
//   The sums follow a bucket's record order: reproducible to the last fp64 bits only, like the normals' moments.
constexpr int kFpfhBins = 11, kFpfhDim = 33, kFpfhRow = 34;   // a row of counts: 33 bins and k
constexpr double kFpfhPi = 3.14159265358979323846;
struct FpfhArgs {
    const float* p; int stride, noff, n;
    float4* pts;              // [n] the eligible points, NaN for the others
    double* nrm;              // [n][4] unit normals
    int* spfh;                // [n][kFpfhRow]
    float* out;               // [n][kFpfhDim]
};
__global__ __launch_bounds__(kNnThreads) void k_fpfh_prep(FpfhArgs a) {
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < a.n; i += gridDim.x * kNnThreads) {
        const float* p = a.p + (size_t)i * a.stride;
        const float x = p[0], y = p[1], z = p[2], nx = p[a.noff], ny = p[a.noff + 1], nz = p[a.noff + 2];
        double ux = 0.0, uy = 0.0, uz = 0.0;
        bool ok = false;
        if (nn_finite(x, y, z) && nn_finite(nx, ny, nz)) {
            const double len = sqrt(((double)nx * (double)nx + (double)ny * (double)ny) + (double)nz * (double)nz);
            if (len > 0.0) { ok = true; ux = (double)nx / len; uy = (double)ny / len; uz = (double)nz / len; }
        }
        a.pts[i] = ok ? make_float4(x, y, z, 0.f) : make_float4(NAN, NAN, NAN, 0.f);
        double* o = a.nrm + (size_t)i * 4;
        o[0] = ux; o[1] = uy; o[2] = uz; o[3] = 0.0;
    }
}
__device__ __forceinline__ int fpfh_bin(double t) { return t >= 10.0 ? 10 : (t > 0.0 ? (int)t : 0); }   // floor, clamped to 0..10
// The bins of the pair (i, j), d = p_j - p_i, unit normals ni and nj; false: the pair is not counted (the header's steps 1 - 5)
__device__ __forceinline__ bool fpfh_pair(double dx, double dy, double dz, double nix, double niy, double niz, double njx, double njy, double njz,
                                          int& b1, int& b2, int& b3) {
    const double L2 = (dx * dx + dy * dy) + dz * dz;
    if (!(L2 > 0.0)) return false;
    const double L = sqrt(L2);
    const double a1 = ((nix * dx + niy * dy) + niz * dz) / L, a2 = ((njx * dx + njy * dy) + njz * dz) / L;
    double n1x = nix, n1y = niy, n1z = niz, n2x = njx, n2y = njy, n2z = njz, f3 = a1;
    if (fabs(a1) < fabs(a2)) {
        n1x = njx; n1y = njy; n1z = njz; n2x = nix; n2y = niy; n2z = niz;
        dx = -dx; dy = -dy; dz = -dz; f3 = -a2;
    }
    double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
    const double vl2 = (vx * vx + vy * vy) + vz * vz;
    if (!(vl2 > 0.0)) return false;
    const double vl = sqrt(vl2);
    vx /= vl; vy /= vl; vz /= vl;
    const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
    const double f2 = (vx * n2x + vy * n2y) + vz * n2z;
    const double f1 = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
    b1 = fpfh_bin(11.0 * (f1 + kFpfhPi) / (2.0 * kFpfhPi));
    b2 = fpfh_bin(11.0 * (f2 + 1.0) / 2.0);
    b3 = fpfh_bin(11.0 * (f3 + 1.0) / 2.0);
    return true;
}
__global__ __launch_bounds__(kNnThreads) void k_fpfh_spfh(NnGrid g, FpfhArgs a) {
    __shared__ int s_h[kFpfhDim][kNnThreads];
    const int tid = threadIdx.x;
    for (int i = blockIdx.x * kNnThreads + tid; i < a.n; i += gridDim.x * kNnThreads) {
        for (int b = 0; b < kFpfhDim; ++b) s_h[b][tid] = 0;
        int k = 0;
        const float4 pi = a.pts[i];
        if (nn_finite(pi.x, pi.y, pi.z)) {
            if (!nn_in_range(g, pi.x, pi.y, pi.z)) atomicOr(g.flag, 1);
            else {
                const double* ni = a.nrm + (size_t)i * 4;
                const double nix = ni[0], niy = ni[1], niz = ni[2];
                nn_walk_records(g, pi.x, pi.y, pi.z, [&](const float4& pj) {
                    const int j = __float_as_int(pj.w);
                    if (j == i) return;
                    const double* nj = a.nrm + (size_t)j * 4;
                    int b1, b2, b3;
                    if (!fpfh_pair((double)pj.x - (double)pi.x, (double)pj.y - (double)pi.y, (double)pj.z - (double)pi.z, nix, niy, niz, nj[0], nj[1],
                                   nj[2], b1, b2, b3))
                        return;
                    ++s_h[b1][tid]; ++s_h[kFpfhBins + b2][tid]; ++s_h[2 * kFpfhBins + b3][tid];
                    ++k;
                });
            }
        }
        int* o = a.spfh + (size_t)i * kFpfhRow;
        for (int b = 0; b < kFpfhDim; ++b) o[b] = s_h[b][tid];
        o[kFpfhDim] = k;
    }
}
constexpr int kFpfhWaves = kNnThreads / 64;   // points per workgroup of k_fpfh_sum
__global__ __launch_bounds__(kNnThreads) void k_fpfh_sum(NnGrid g, FpfhArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bin = min(lane, kFpfhDim - 1);      // (the lanes past the last bin walk along and store nothing)
    for (int i0 = blockIdx.x * kFpfhWaves; i0 < a.n; i0 += gridDim.x * kFpfhWaves) {
        const int i = i0 + wave;
        if (i >= a.n) continue;
        double acc = 0.0;
        const float4 pi = a.pts[i];
        if (nn_finite(pi.x, pi.y, pi.z) && nn_in_range(g, pi.x, pi.y, pi.z)) {
            nn_walk_records(g, pi.x, pi.y, pi.z, [&](const float4& pj) {
                const int j = __float_as_int(pj.w);
                if (j == i) return;
                const int* sj = a.spfh + (size_t)j * kFpfhRow;
                const int kj = sj[kFpfhDim];
                if (kj <= 0) return;
                const double dx = (double)pj.x - (double)pi.x, dy = (double)pj.y - (double)pi.y, dz = (double)pj.z - (double)pi.z;
                const double L2 = (dx * dx + dy * dy) + dz * dz;
                if (!(L2 > 0.0)) return;
                acc += ((1.0 / L2) / (double)kj) * (double)sj[bin];
            });
        }
        double p0 = 0.0, p1 = 0.0, p2 = 0.0;      // the parts' sums, every lane the same: bins in order
#pragma unroll
        for (int m = 0; m < kFpfhDim; ++m) {
            const double v = __shfl(acc, m, 64);
            if (m < kFpfhBins) p0 += v;
            else if (m < 2 * kFpfhBins) p1 += v;
            else p2 += v;
        }
        const bool ok = p0 > 0.0 && p1 > 0.0 && p2 > 0.0;
        const double part = lane < kFpfhBins ? p0 : (lane < 2 * kFpfhBins ? p1 : p2);
        if (lane < kFpfhDim) a.out[(size_t)i * kFpfhDim + lane] = ok ? (float)(100.0 * acc / part) : NAN;
    }
}

// ---------------- nearest descriptor (mf_feature_match_dev; DESIGN.md "Global registration") ----------------
// Brute force: one lane per query, one workgroup per kMatchThreads queries.  A lane's query row sits in LDS as float4 groups, group-major
// (s_q[group][lane]: 16 contiguous bytes a lane, no conflicts), padded with zeros to a multiple of four bins; the targets pass through LDS in
// tiles of kMatchTile rows, padded the same way, and every lane reads the same target group (a broadcast).  A padded bin adds (0 - 0)^2 = +0
// to a sum that is >= +0 or NaN: the fp32 d2 is that of the dim bins in order.  Targets are scanned in index order and only a strictly
// smaller d2 replaces the best, so ties go to the smallest index, a row with a NaN (d2 = NaN) never wins and a query with a NaN keeps -1, +inf.
constexpr int kMatchThreads = 128, kMatchTile = 64, kMatchMaxDim = 64;
struct MatchArgs {
    const float* t; int nt;
    const float* q; int nq;
    int dim;
    int* idx; float* d2;
};
__global__ __launch_bounds__(kMatchThreads) void k_feature_match(MatchArgs a) {
    __shared__ float4 s_q[kMatchMaxDim / 4][kMatchThreads];
    __shared__ float4 s_t[kMatchTile][kMatchMaxDim / 4];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kMatchThreads + tid;
    const int d4 = (a.dim + 3) >> 2;
    for (int c = 0; c < d4; ++c) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = 4 * c + k;
            v[k] = (i < a.nq && b < a.dim) ? a.q[(size_t)i * a.dim + b] : 0.f;
        }
        s_q[c][tid] = make_float4(v[0], v[1], v[2], v[3]);
    }
    float best = INFINITY;
    int bj = -1;
    float* st = (float*)s_t;
    for (int t0 = 0; t0 < a.nt; t0 += kMatchTile) {
        const int rows = min(kMatchTile, a.nt - t0);
        __syncthreads();       // the tile before has been read
        for (int e = tid; e < rows * d4 * 4; e += kMatchThreads) {
            const int r = e / (d4 * 4), b = e - r * (d4 * 4);
            st[r * kMatchMaxDim + b] = b < a.dim ? a.t[(size_t)(t0 + r) * a.dim + b] : 0.f;
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            float d2 = 0.f;
            for (int c = 0; c < d4; ++c) {
                const float4 q = s_q[c][tid], t = s_t[r][c];
                const float dx = q.x - t.x, dy = q.y - t.y, dz = q.z - t.z, dw = q.w - t.w;
                d2 = d2 + dx * dx;
                d2 = d2 + dy * dy;
                d2 = d2 + dz * dz;
                d2 = d2 + dw * dw;
            }
            if (d2 < best) { best = d2; bj = t0 + r; }
        }
    }
    if (i < a.nq) { a.idx[i] = bj; a.d2[i] = best; }
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
// the three checks every entry point shares
static bool nn_radius_ok(float radius) { return std::isfinite(radius) && radius > 0.f; }
static bool nn_count_ok(int64_t n) { return n >= 0 && n <= (int64_t)1 << 30; }
static bool nn_ws_ok(const void* d_ws, uint64_t bytes, uint64_t need) { return d_ws && ((uintptr_t)d_ws & 15) == 0 && bytes >= need; }
// workspace: rec [N] float4 | start [B + 1] | rank [N] | sums [kNnScanBlocks] | flag
uint64_t nn_workspace_bytes(int64_t n_target) {
    const uint64_t n = (uint64_t)std::max<int64_t>(n_target, 0);
    return nn_align(n * 16) + nn_align((nn_buckets(n_target) + 1) * 4) + nn_align(n * 4) + nn_align(kNnScanBlocks * 4) + 256;
}
static int nn_grid_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kNnThreads - 1) / kNnThreads, kNnMaxGrid)); }

// the grid of n_target targets and `radius` laid out in a workspace of nn_workspace_bytes(n_target)
NnGrid nn_layout(void* d_ws, int64_t n_target, float radius) {
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
static int nn_fail(const char** why, const char* text, int rc) {
    if (why) *why = text;
    return rc;
}
// clears the flag and fills the grid (count, scan, scatter); normal_offset >= 0: the normals go to nrm by record slot
// (why, here and in nn_finish: where the text of a failure goes, or null -- only nn_run's caller reads it)
int nn_build(const NnGrid& g, const float* d_target, int target_stride, int normal_offset, float4* nrm, int64_t n_target, hipStream_t s,
             const char** why) {
    const uint64_t B = (uint64_t)g.mask + 1;
    if (hipMemsetAsync(g.start, 0, (B + 1) * 4, s) != hipSuccess || hipMemsetAsync(g.flag, 0, sizeof(int), s) != hipSuccess) return nn_fail(why, "hipMemsetAsync failed", MF_EHIP);
    if (n_target > 0) {
        const int nb = nn_grid_blocks(n_target);
        hipLaunchKernelGGL(k_nn_count, dim3(nb), dim3(kNnThreads), 0, s, d_target, target_stride, normal_offset, (int)n_target, g);
        hipLaunchKernelGGL(k_nn_scan_sums, dim3(kNnScanBlocks), dim3(kNnThreads), 0, s, g, (unsigned)B);
        hipLaunchKernelGGL(k_nn_scan_apply, dim3(kNnScanBlocks), dim3(kNnThreads), 0, s, g, (unsigned)B);
        hipLaunchKernelGGL(k_nn_scatter, dim3(nb), dim3(kNnThreads), 0, s, d_target, target_stride, normal_offset, nrm, (int)n_target, g);
    }
    return MF_OK;
}
// (mf_mesh.hip compacts its block directory and its vertex and quad flags with the same two launches)
void nn_exclusive_scan(unsigned* d, unsigned* sums, unsigned n, hipStream_t s) {
    NnGrid g;
    memset(&g, 0, sizeof(g));
    g.start = d; g.sums = sums;
    hipLaunchKernelGGL(k_nn_scan_sums, dim3(kNnScanBlocks), dim3(kNnThreads), 0, s, g, n);
    hipLaunchKernelGGL(k_nn_scan_apply, dim3(kNnScanBlocks), dim3(kNnThreads), 0, s, g, n);
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
int nn_finish(const NnGrid& g, hipStream_t s, const char** why) {
    if (hipGetLastError() != hipSuccess) return nn_fail(why, "kernel launch failed", MF_EHIP);
    int flag = 0;
    if (hipMemcpyAsync(&flag, g.flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return nn_fail(why, "HIP error during the nearest-neighbour kernels", MF_EHIP);
    if (flag) return nn_fail(why, "a coordinate has |x / radius| >= 2^30", MF_EINVAL);
    return MF_OK;
}

int nn_run(const float* d_target, int target_stride, int64_t n_target, const float* d_query, int query_stride, int64_t n_query,
           const float* T16, float radius, float* d_dist, int32_t* d_idx, void* d_ws, uint64_t ws_bytes, hipStream_t s, const char** why) {
    if (!nn_radius_ok(radius)) return nn_fail(why, "radius must be finite and > 0", MF_EINVAL);
    if (target_stride < 3 || query_stride < 3) return nn_fail(why, "strides must be >= 3 floats", MF_EINVAL);
    if (!nn_count_ok(n_target) || !nn_count_ok(n_query)) return nn_fail(why, "point count out of range", MF_EINVAL);
    if ((n_target > 0 && !d_target) || (n_query > 0 && (!d_query || !d_dist || !d_idx))) return nn_fail(why, "null pointer", MF_EINVAL);
    if (!nn_ws_ok(d_ws, ws_bytes, nn_workspace_bytes(n_target))) return nn_fail(why, "workspace missing, misaligned or too small", MF_EINVAL);
    if (T16 && !nn_transform_finite(T16)) return nn_fail(why, "transform is not finite", MF_EINVAL);
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

static int icp_build(const float* d_target, int target_stride, int normal_offset, int64_t n_target, float radius, void* d_ws, uint64_t ws_bytes,
                     hipStream_t s) {
    if (!nn_radius_ok(radius)) return MF_EINVAL;
    if (target_stride < 3 || (normal_offset >= 0 && (normal_offset < 3 || normal_offset + 3 > target_stride))) return MF_EINVAL;
    if (!nn_count_ok(n_target) || (n_target > 0 && !d_target)) return MF_EINVAL;
    if (!nn_ws_ok(d_ws, ws_bytes, icp_workspace_bytes(n_target, 0))) return MF_EINVAL;
    char* w = (char*)d_ws;
    // not a built workspace until the build has gone through
    if (hipMemsetAsync(w, 0, 256, s) != hipSuccess) return MF_EHIP;
    const NnGrid g = nn_layout(w + 256, n_target, radius);
    float4* nrm = (float4*)(w + 256 + nn_workspace_bytes(n_target));
    int rc = nn_build(g, d_target, target_stride, normal_offset < 0 ? -1 : normal_offset, nrm, n_target, s);
    if (rc != MF_OK) return rc;
    rc = nn_finish(g, s);
    if (rc != MF_OK) return rc;
    const IcpHeader h = {kIcpMagic, n_target, radius, normal_offset >= 0 ? 1 : 0};
    if (hipMemcpyAsync(w, &h, sizeof(h), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return MF_EHIP;
    return MF_OK;
}

static int icp_step(void* d_ws, uint64_t ws_bytes, const float* d_query, int query_stride, int64_t n_query, const float* T16, double* d_out29,
                    hipStream_t s) {
    if (query_stride < 3 || !nn_count_ok(n_query) || (n_query > 0 && !d_query) || !d_out29) return MF_EINVAL;
    if (!nn_ws_ok(d_ws, ws_bytes, 256)) return MF_EINVAL;
    if (T16 && !nn_transform_finite(T16)) return MF_EINVAL;
    char* w = (char*)d_ws;
    IcpHeader h;
    if (hipMemcpyAsync(&h, w, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return MF_EHIP;
    if (h.magic != kIcpMagic || !nn_count_ok(h.n_target) || !nn_radius_ok(h.radius)) return MF_EINVAL;
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
    return nn_finish(g, s);
}

// ---------------- normals: workspace = the grid's workspace | sums [9][n] double ----------------
static uint64_t normals_workspace_bytes(int64_t n) { return nn_workspace_bytes(n) + nn_align((uint64_t)std::max<int64_t>(n, 0) * 72); }
static int normals_run(const float* d_points, int stride, int64_t n, float radius, int min_neighbours, const float* viewpoint3, float4* d_normals,
                       int32_t* d_count, void* d_ws, uint64_t ws_bytes, hipStream_t s) {
    if (!nn_radius_ok(radius) || stride < 3 || min_neighbours < 3) return MF_EINVAL;
    if (!nn_count_ok(n) || (n > 0 && (!d_points || !d_normals || !d_count))) return MF_EINVAL;
    if (!nn_ws_ok(d_ws, ws_bytes, normals_workspace_bytes(n))) return MF_EINVAL;
    if (viewpoint3 && !(std::isfinite(viewpoint3[0]) && std::isfinite(viewpoint3[1]) && std::isfinite(viewpoint3[2]))) return MF_EINVAL;
    const NnGrid g = nn_layout(d_ws, n, radius);
    const int rc = nn_build(g, d_points, stride, -1, nullptr, n, s);
    if (rc != MF_OK) return rc;
    if (n > 0) {
        NrmArgs a;
        memset(&a, 0, sizeof(a));
        a.p = d_points; a.stride = stride; a.n = (int)n; a.min_k = min_neighbours; a.out = d_normals; a.count = d_count;
        if (viewpoint3) { a.has_view = 1; memcpy(a.view, viewpoint3, sizeof(a.view)); }
        double* sums = (double*)((char*)d_ws + nn_workspace_bytes(n));
        hipLaunchKernelGGL(k_normals_walk, dim3(nn_grid_blocks(n)), dim3(kNnThreads), 0, s, g, a, sums);
        hipLaunchKernelGGL(k_normals_solve, dim3(nn_grid_blocks(n)), dim3(kNnThreads), 0, s, a, (const double*)sums);
    }
    return nn_finish(g, s);
}

// ---------------- FPFH: workspace = points [n] float4 | normals [n][4] double | the grid's workspace | counts [n][34] int ----------------
static uint64_t fpfh_grid_at(int64_t n) { const uint64_t N = (uint64_t)std::max<int64_t>(n, 0); return nn_align(N * 16) + nn_align(N * 32); }
static uint64_t fpfh_workspace_bytes(int64_t n) {
    return fpfh_grid_at(n) + nn_workspace_bytes(n) + nn_align((uint64_t)std::max<int64_t>(n, 0) * kFpfhRow * 4);
}
static int fpfh_run(const float* d_points, int stride, int normal_offset, int64_t n, float radius, float* d_fpfh, int32_t* d_spfh, void* d_ws,
                    uint64_t ws_bytes, hipStream_t s) {
    if (!nn_radius_ok(radius) || stride < 6 || normal_offset < 3 || normal_offset + 3 > stride) return MF_EINVAL;
    if (!nn_count_ok(n) || (n > 0 && (!d_points || !d_fpfh))) return MF_EINVAL;
    if (!nn_ws_ok(d_ws, ws_bytes, fpfh_workspace_bytes(n))) return MF_EINVAL;
    char* w = (char*)d_ws;
    FpfhArgs a;
    memset(&a, 0, sizeof(a));
    a.p = d_points; a.stride = stride; a.noff = normal_offset; a.n = (int)n; a.out = d_fpfh;
    a.pts = (float4*)w;
    a.nrm = (double*)(w + nn_align((uint64_t)n * 16));
    a.spfh = d_spfh ? d_spfh : (int*)(w + fpfh_grid_at(n) + nn_workspace_bytes(n));
    const NnGrid g = nn_layout(w + fpfh_grid_at(n), n, radius);
    if (n > 0) hipLaunchKernelGGL(k_fpfh_prep, dim3(nn_grid_blocks(n)), dim3(kNnThreads), 0, s, a);
    const int rc = nn_build(g, (const float*)a.pts, 4, -1, nullptr, n, s);
    if (rc != MF_OK) return rc;
    if (n > 0) {
        hipLaunchKernelGGL(k_fpfh_spfh, dim3(nn_grid_blocks(n)), dim3(kNnThreads), 0, s, g, a);
        const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n + kFpfhWaves - 1) / kFpfhWaves, kNnMaxGrid));
        hipLaunchKernelGGL(k_fpfh_sum, dim3(nb), dim3(kNnThreads), 0, s, g, a);
    }
    return nn_finish(g, s);
}

static int feature_match(const float* d_target, int64_t n_target, const float* d_query, int64_t n_query, int dim, int32_t* d_idx, float* d_d2,
                         hipStream_t s) {
    if (dim < 1 || dim > kMatchMaxDim) return MF_EINVAL;
    if (!nn_count_ok(n_target) || !nn_count_ok(n_query)) return MF_EINVAL;
    if ((n_target > 0 && !d_target) || (n_query > 0 && (!d_query || !d_idx || !d_d2))) return MF_EINVAL;
    if (n_query > 0) {
        MatchArgs a;
        memset(&a, 0, sizeof(a));
        a.t = d_target; a.nt = (int)n_target; a.q = d_query; a.nq = (int)n_query; a.dim = dim; a.idx = d_idx; a.d2 = d_d2;
        hipLaunchKernelGGL(k_feature_match, dim3((unsigned)((n_query + kMatchThreads - 1) / kMatchThreads)), dim3(kMatchThreads), 0, s, a);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return MF_EHIP;
    return MF_OK;
}

}  // namespace mf

using namespace mf;

extern "C" int mf_cloud_nn_workspace(int64_t n_target, uint64_t* bytes) {
    if (!bytes || !nn_count_ok(n_target)) return MF_EINVAL;
    *bytes = nn_workspace_bytes(n_target);
    return MF_OK;
}

extern "C" int mf_cloud_nn_dev(const float* d_target, int32_t target_stride, int64_t n_target, const float* d_query, int32_t query_stride, int64_t n_query,
                               const float* query_to_target16, float radius, float* d_dist, int32_t* d_idx, void* d_workspace, uint64_t workspace_bytes,
                               void* stream) {
    return nn_run(d_target, target_stride, n_target, d_query, query_stride, n_query, query_to_target16, radius, d_dist, d_idx, d_workspace,
                  workspace_bytes, (hipStream_t)stream, nullptr);
}

extern "C" int mf_cloud_icp_workspace(int64_t n_target, int64_t n_query, uint64_t* bytes) {
    if (!bytes || !nn_count_ok(n_target) || !nn_count_ok(n_query)) return MF_EINVAL;
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

extern "C" int mf_cloud_normals_workspace(int64_t n, uint64_t* bytes) {
    if (!bytes || !nn_count_ok(n)) return MF_EINVAL;
    *bytes = normals_workspace_bytes(n);
    return MF_OK;
}

extern "C" int mf_cloud_normals_dev(const float* d_points, int32_t stride, int64_t n, float radius, int32_t min_neighbours, const float* viewpoint3,
                                    float* d_normals, int32_t* d_count, void* d_workspace, uint64_t workspace_bytes, void* stream) {
    return normals_run(d_points, stride, n, radius, min_neighbours, viewpoint3, (float4*)d_normals, d_count, d_workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int mf_cloud_fpfh_workspace(int64_t n, uint64_t* bytes) {
    if (!bytes || !nn_count_ok(n)) return MF_EINVAL;
    *bytes = fpfh_workspace_bytes(n);
    return MF_OK;
}

extern "C" int mf_cloud_fpfh_dev(const float* d_points, int32_t stride, int32_t normal_offset, int64_t n, float radius, float* d_fpfh, int32_t* d_spfh,
                                 void* d_workspace, uint64_t workspace_bytes, void* stream) {
    return fpfh_run(d_points, stride, normal_offset, n, radius, d_fpfh, d_spfh, d_workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int mf_feature_match_dev(const float* d_target, int64_t n_target, const float* d_query, int64_t n_query, int32_t dim, int32_t* d_idx,
                                    float* d_d2, void* stream) {
    return feature_match(d_target, n_target, d_query, n_query, dim, d_idx, d_d2, (hipStream_t)stream);
}
