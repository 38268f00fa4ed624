// mf_register.hip -- the hypothesis search of a registration without a start (mf_pose_ransac_dev; DESIGN.md "Inactive models and
// re-detection"): h triples of correspondences, each checked, fitted in closed form and scored against all m correspondences.  No upstream twin:
// the reference declares Model::detectInRegion and ships it empty.  Fourth file of the evaluation family; it shares nothing with the others but
// the compile flag below, and it needs no context.
//
// Shape: three launches on the caller's stream, no workspace, no wait.
//   1. k_ransac_score, grid (ceil(h / 256), chunks of kRansacChunk correspondences): a lane per hypothesis.  The lane checks and fits its
//      triple once, before its first tile, and keeps R, t (12 doubles) in registers; the workgroup's chunk of the correspondences passes through
//      LDS in tiles of kRansacTile, already widened to fp64 (six doubles a correspondence), and every lane reads the same address (a broadcast).
//      A lane's count over the chunk goes into d_counts with one integer atomicAdd; the call zeroes d_counts first.  blockIdx.y == 0 writes
//      the statuses.  (20 000 hypotheses are 79 workgroups: the split over blockIdx.y is what fills the machine.)
//   2. k_ransac_pick, one workgroup: the largest (count, smallest index) among the tested triples -> d_best.
//   3. k_ransac_mask, a lane per correspondence: thread 0 of every workgroup fits the winner again (the same device function on the same
//      values: the same bits), the lanes write the mask, workgroup 0 writes the pose.
// Everything that decides anything is an integer count or an index, so the result does not depend on the order of execution.  The fp64
// arithmetic is rounded operation by operation in the order the header gives: this file is compiled without contraction (-ffp-contract=off,
// and the pragma for a build that forgets the flag).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/maskfusion_amd.h"
#include "mf_internal.h"

namespace mf {

constexpr int kRansacThreads = 256;        // hypotheses a workgroup
constexpr int kRansacTile = 128;           // correspondences a tile: 6 KB of LDS
constexpr int kRansacChunk = 2048;         // correspondences a workgroup (blockIdx.y): 16 tiles
constexpr int kRansacMax = 1 << 24;        // m and h: counts stay exact in every integer type used, gridDim.y <= 8192

struct RansacArgs {
    const float* src; const float* dst;
    int stride, m;
    const int* tri; int h;
    double thr2, keep;                     // inlier_distance^2 and 1 - edge_tolerance, both formed once on the host
    unsigned* counts; unsigned char* status; int* best; unsigned char* inlier; double* pose;
};

struct Pose { double r[3][4]; };           // rows R_r0 R_r1 R_r2 t_r

__device__ __forceinline__ double len3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// the status of a triple and, for status 0, its pose (header: "Status", "Fit")
__device__ __forceinline__ int ransac_fit(const RansacArgs& a, int j, Pose& P) {
    const int i0 = a.tri[3 * (size_t)j], i1 = a.tri[3 * (size_t)j + 1], i2 = a.tri[3 * (size_t)j + 2];
    if (i0 < 0 || i0 >= a.m || i1 < 0 || i1 >= a.m || i2 < 0 || i2 >= a.m || i0 == i1 || i0 == i2 || i1 == i2) return 1;
    double s[3][3], d[3][3];
    const int idx[3] = {i0, i1, i2};
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float u = a.src[(size_t)idx[k] * a.stride + c], v = a.dst[(size_t)idx[k] * a.stride + c];
            finite = finite && fabsf(u) <= 3.402823466e38f && fabsf(v) <= 3.402823466e38f;          // a NaN fails
            s[k][c] = (double)u;
            d[k][c] = (double)v;
        }
    if (!finite) return 3;
    const int ea[3] = {0, 0, 1}, eb[3] = {1, 2, 2};
    bool edges = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const double ls = len3(s[eb[e]][0] - s[ea[e]][0], s[eb[e]][1] - s[ea[e]][1], s[eb[e]][2] - s[ea[e]][2]);
        const double ld = len3(d[eb[e]][0] - d[ea[e]][0], d[eb[e]][1] - d[ea[e]][1], d[eb[e]][2] - d[ea[e]][2]);
        const double lo = ls < ld ? ls : ld, hi = ls < ld ? ld : ls;
        edges = edges && lo > 0.0 && lo >= a.keep * hi;
    }
    if (!edges) return 2;
    double B[2][3][3];                     // the frames e1 e2 e3 of src and f1 f2 f3 of dst, as rows
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const double (*p)[3] = side ? d : s;
        const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
        const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
        const double wx = ay * bz - az * by, wy = az * bx - ax * bz, wz = ax * by - ay * bx;
        const double la = len3(ax, ay, az), lw = len3(wx, wy, wz);
        if (lw == 0.0) return 3;
        double* e1 = B[side][0];
        double* e2 = B[side][1];
        double* e3 = B[side][2];
        e1[0] = ax / la; e1[1] = ay / la; e1[2] = az / la;
        e3[0] = wx / lw; e3[1] = wy / lw; e3[2] = wz / lw;
        e2[0] = e3[1] * e1[2] - e3[2] * e1[1];
        e2[1] = e3[2] * e1[0] - e3[0] * e1[2];
        e2[2] = e3[0] * e1[1] - e3[1] * e1[0];
    }
    double cs[3], cd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cs[c] = ((s[0][c] + s[1][c]) + s[2][c]) / 3.0;
        cd[c] = ((d[0][c] + d[1][c]) + d[2][c]) / 3.0;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) P.r[r][c] = (B[1][0][r] * B[0][0][c] + B[1][1][r] * B[0][1][c]) + B[1][2][r] * B[0][2][c];
        P.r[r][3] = cd[r] - ((P.r[r][0] * cs[0] + P.r[r][1] * cs[1]) + P.r[r][2] * cs[2]);
    }
    return 0;
}

// header: "Score".  A NaN anywhere fails the comparison.
__device__ __forceinline__ bool ransac_inlier(const Pose& P, double x, double y, double z, double u, double v, double w, double thr2) {
    const double dx = (((P.r[0][0] * x + P.r[0][1] * y) + P.r[0][2] * z) + P.r[0][3]) - u;
    const double dy = (((P.r[1][0] * x + P.r[1][1] * y) + P.r[1][2] * z) + P.r[1][3]) - v;
    const double dz = (((P.r[2][0] * x + P.r[2][1] * y) + P.r[2][2] * z) + P.r[2][3]) - w;
    return (dx * dx + dy * dy) + dz * dz <= thr2;
}

__global__ __launch_bounds__(kRansacThreads) void k_ransac_score(RansacArgs a) {
    __shared__ double s_c[kRansacTile][6];
    const int tid = threadIdx.x;
    const int j = blockIdx.x * kRansacThreads + tid;
    Pose P;
    int status = 1;
    if (j < a.h) {
        status = ransac_fit(a, j, P);
        if (blockIdx.y == 0) a.status[j] = (unsigned char)status;
    }
    const bool tested = j < a.h && status == 0;
    const int k0 = blockIdx.y * kRansacChunk, k1 = min(a.m, k0 + kRansacChunk);
    unsigned cnt = 0u;
    for (int t0 = k0; t0 < k1; t0 += kRansacTile) {
        const int rows = min(kRansacTile, k1 - t0);
        __syncthreads();                   // the tile before has been read
        for (int e = tid; e < rows * 6; e += kRansacThreads) {
            const int r = e / 6, c = e - r * 6;
            const float* p = (c < 3 ? a.src : a.dst) + (size_t)(t0 + r) * a.stride + (c < 3 ? c : c - 3);
            s_c[r][c] = (double)*p;
        }
        __syncthreads();
        if (tested)
            for (int r = 0; r < rows; ++r)
                cnt += ransac_inlier(P, s_c[r][0], s_c[r][1], s_c[r][2], s_c[r][3], s_c[r][4], s_c[r][5], a.thr2) ? 1u : 0u;
    }
    if (tested && cnt) atomicAdd(&a.counts[j], cnt);
}

// the tested triple with the largest count, ties to the smallest index: the maximum of (count + 1) << 32 | ~index; 0: no tested triple
__global__ __launch_bounds__(kRansacThreads) void k_ransac_pick(RansacArgs a) {
    __shared__ unsigned long long s_key[kRansacThreads];
    const int tid = threadIdx.x;
    unsigned long long key = 0ull;
    for (int j = tid; j < a.h; j += kRansacThreads) {
        if (a.status[j] != 0) continue;
        const unsigned long long k = ((unsigned long long)(a.counts[j] + 1u) << 32) | (unsigned long long)(0xffffffffu - (unsigned)j);
        if (k > key) key = k;
    }
    s_key[tid] = key;
    __syncthreads();
    for (int w = kRansacThreads / 2; w > 0; w >>= 1) {
        if (tid < w && s_key[tid + w] > s_key[tid]) s_key[tid] = s_key[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        key = s_key[0];
        a.best[0] = key ? (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)) : -1;
        a.best[1] = key ? (int)((unsigned)(key >> 32) - 1u) : 0;
    }
}

__global__ __launch_bounds__(kRansacThreads) void k_ransac_mask(RansacArgs a) {
    __shared__ Pose s_P;
    const int j = a.best[0];
    if (threadIdx.x == 0 && j >= 0) {
        Pose P;
        ransac_fit(a, j, P);               // status 0, as in k_ransac_score
        s_P = P;
        if (blockIdx.x == 0 && a.pose)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) a.pose[4 * r + c] = P.r[r][c];
    }
    __syncthreads();
    const int k = blockIdx.x * kRansacThreads + threadIdx.x;
    if (k >= a.m || !a.inlier) return;
    bool in = false;
    if (j >= 0) {
        const float* p = a.src + (size_t)k * a.stride;
        const float* q = a.dst + (size_t)k * a.stride;
        in = ransac_inlier(s_P, (double)p[0], (double)p[1], (double)p[2], (double)q[0], (double)q[1], (double)q[2], a.thr2);
    }
    a.inlier[k] = in ? 1 : 0;
}

static int pose_ransac(const float* d_src, const float* d_dst, int32_t stride, int32_t m, const int32_t* d_triples, int32_t h, double inlier_distance,
                       double edge_tolerance, uint32_t* d_counts, uint8_t* d_status, int32_t* d_best, uint8_t* d_inlier, double* d_pose, hipStream_t s) {
    if (stride < 3 || m < 0 || m > kRansacMax || h < 0 || h > kRansacMax) return MF_EINVAL;
    if (!std::isfinite(inlier_distance) || !(inlier_distance > 0.0)) return MF_EINVAL;
    if (!(edge_tolerance >= 0.0 && edge_tolerance < 1.0)) return MF_EINVAL;          // a NaN fails
    if (m > 0 && h > 0 && (!d_src || !d_dst || !d_triples || !d_counts || !d_status || !d_best)) return MF_EINVAL;
    // from here on a null pointer means m == 0 or h == 0.  Without correspondences no triple reads a point (status 1), so only the triples'
    // own arrays have to be there; without them, or without triples, there is nothing to score
    if (h > 0 && (!d_triples || !d_counts || !d_status)) h = 0;
    RansacArgs a;
    a.src = d_src; a.dst = d_dst; a.stride = stride; a.m = m; a.tri = d_triples; a.h = h;
    a.thr2 = inlier_distance * inlier_distance;
    a.keep = 1.0 - edge_tolerance;
    a.counts = d_counts; a.status = d_status; a.best = d_best; a.inlier = d_inlier; a.pose = d_pose;
    if (h > 0) {
        if (hipMemsetAsync(d_counts, 0, (size_t)h * sizeof(uint32_t), s) != hipSuccess) return MF_EHIP;
        const unsigned gx = (unsigned)((h + kRansacThreads - 1) / kRansacThreads);                // at most 2^16
        const unsigned gy = (unsigned)std::max(1, (m + kRansacChunk - 1) / kRansacChunk);           // at most 2^13
        hipLaunchKernelGGL(k_ransac_score, dim3(gx, gy), dim3(kRansacThreads), 0, s, a);
    }
    if (d_best) hipLaunchKernelGGL(k_ransac_pick, dim3(1), dim3(kRansacThreads), 0, s, a);
    if (d_best && m > 0 && (d_inlier || d_pose))
        hipLaunchKernelGGL(k_ransac_mask, dim3((unsigned)((m + kRansacThreads - 1) / kRansacThreads)), dim3(kRansacThreads), 0, s, a);
    return hipGetLastError() == hipSuccess ? MF_OK : MF_EHIP;
}

}  // namespace mf

using namespace mf;

extern "C" int mf_pose_ransac_dev(const float* d_src, const float* d_dst, int32_t stride, int32_t m, const int32_t* d_triples, int32_t h,
                                  double inlier_distance, double edge_tolerance, uint32_t* d_counts, uint8_t* d_status, int32_t* d_best,
                                  uint8_t* d_inlier, double* d_pose, void* stream) {
    return pose_ransac(d_src, d_dst, stride, m, d_triples, h, inlier_distance, edge_tolerance, d_counts, d_status, d_best, d_inlier, d_pose,
                       (hipStream_t)stream);
}
