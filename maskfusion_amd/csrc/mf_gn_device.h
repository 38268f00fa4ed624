// mf_gn_device.h -- the parts of a Gauss-Newton step of the tracker that the three loops of mf_odometry.hip (geometric for one model, geometric
// batched, RGB-D) share, each written once: the fixed-order reductions, the per-pixel arithmetic of the geometric term, and gn_seed, gn_stage,
// gn_publish, icp_slots, store_block_partial, pose_from_state.  The loops must agree bit for bit (tests/test_gpu_multimodel.py); they do because
// they call the same functions, not copies of them.  The solve itself (ldlt6_solve ... gn_finish_wg, gn_step_wg) stays in mf_odometry.hip: the
// host-compiled and the CPU-executed test builds read that file's text.  DESIGN.md: "One Gauss-Newton step".
#pragma once

#include "mf_internal.h"
#include "mf_device.h"

namespace mf {

// value of lane (lane ^ kXor) for a 32-bit pattern, kXor = 1 or 2: quad permutes on the DPP path (no LDS crossbar)
template <int kXor>
__device__ __forceinline__ float lane_xor_bits(int bits, int /*lane*/) {
    static_assert(kXor == 1 || kXor == 2, "quad permutes only");
    return __int_as_float(__builtin_amdgcn_update_dpp(0, bits, kXor == 1 ? 0xB1 : 0x4E, 0xf, 0xf, false));
}

// Fixed-order reduction of `nb` per-workgroup partials ([nb][32] floats) by a 256-thread workgroup -> sys[32] doubles
// in LDS.  The array is read as float4s with up to 10 independent 16 B loads in flight per lane (a one-load-at-a-time
// loop cost ~70 cycles per partial: 10 us at 300 workgroups; the partials live in other XCDs' L2s, so every batch is
// a fabric round trip).  Thread t < 256 owns components 4*(t%8)..+3 of workgroups t/8, t/8 + 32, ...
// Round 4 (in-kernel stamps, profiles/r04c_icp_prof.txt: this phase was 3.1 k of a launch's 13.6 k ticks, of which the memory round trip
// is ~0.9 k): a thread's own <= 10 values per component are added in fp32 -- they ARE fp32 sums of up to 1 536 products each, the extra
// rounding is below theirs -- instead of 40 conversions + 40 fp64 additions + 80 selects per thread on a quarter-rate pipe; the 32 row sums
// per component are then added in fp64 by FOUR lanes per component (8 rows each, in row order) and a quad butterfly on the DPP path
// instead of one lane walking 32 dependent additions.  The order is fixed, so every workgroup (and every run) gets bit-identical sums.
__device__ __forceinline__ double quad_sum_d(double v) {   // v + its three quad neighbours, same bits in all four lanes
    const int lane = threadIdx.x & 63;
    int lo = __double2loint(v), hi = __double2hiint(v);
    double o = __hiloint2double(__float_as_int(lane_xor_bits<1>(hi, lane)), __float_as_int(lane_xor_bits<1>(lo, lane)));
    v = (lane & 1) ? o + v : v + o;            // both lanes of a pair add (even lane's value) + (odd lane's value)
    lo = __double2loint(v); hi = __double2hiint(v);
    o = __hiloint2double(__float_as_int(lane_xor_bits<2>(hi, lane)), __float_as_int(lane_xor_bits<2>(lo, lane)));
    return (lane & 2) ? o + v : v + o;
}
__device__ __forceinline__ void reduce_rows(const double* s_seg /*[32][32]*/, double* s_sys /*[32]*/, int t /* 0..127 */) {
    const int comp = t >> 2, part = t & 3;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += s_seg[(part * 8 + k) * 32 + comp];
    s = quad_sum_d(s);
    if (part == 0) s_sys[comp] = s;
}
__device__ __forceinline__ void partial_sums_f32(const float4* __restrict__ p4, int n4, int t, float (&a)[4]) {
    a[0] = a[1] = a[2] = a[3] = 0.f;
    for (int f = t; f < n4; f += 2560) {  // 10 independent 16 B loads in flight per lane
        float4 v[10];
#pragma unroll
        for (int u = 0; u < 10; ++u) v[u] = p4[min(f + 256 * u, n4 - 1)];  // unconditional: all ten issue back to back
#pragma unroll
        for (int u = 0; u < 10; ++u) {
            const bool in = f + 256 * u < n4;
            a[0] += in ? v[u].x : 0.f; a[1] += in ? v[u].y : 0.f;
            a[2] += in ? v[u].z : 0.f; a[3] += in ? v[u].w : 0.f;
        }
    }
}
__device__ __forceinline__ void reduce_partials(const float* __restrict__ partials, int nb, double* s_seg /*[32][32]*/,
                                                double* s_sys /*[32]*/) {
    // The first 256 threads of the workgroup load; any workgroup size that is a multiple of 256 may call this.
    if (threadIdx.x < 256) {
        float a[4];
        partial_sums_f32(reinterpret_cast<const float4*>(partials), nb * (kIcpSlots / 4), threadIdx.x, a);
        const int row = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
        s_seg[row * 32 + c4 + 0] = (double)a[0]; s_seg[row * 32 + c4 + 1] = (double)a[1];
        s_seg[row * 32 + c4 + 2] = (double)a[2]; s_seg[row * 32 + c4 + 3] = (double)a[3];
    }
    __syncthreads();
    if (threadIdx.x < 128) reduce_rows(s_seg, s_sys, threadIdx.x);
    __syncthreads();
}

// Two partial arrays (ICP and photometric) and the correspondence counts in ONE memory latency: threads 0..255 reduce the
// first array, threads 256..511 the second, wavefront 0 issues the count loads ahead of its partial loads.  Needs a
// workgroup of >= 512 threads (the kernels here have exactly that); bit-identical sums to two reduce_partials calls.
__device__ __forceinline__ void reduce_partials_pair(const float* __restrict__ pa, const float* __restrict__ pb, const int2* __restrict__ cnt,
                                                     int nb, double* s_segA, double* s_segB, double* s_sysA, double* s_sysB, int* s_cnt) {
    const int half = threadIdx.x >> 8, t = threadIdx.x & 255;
    unsigned c = 0, g = 0;
    if (threadIdx.x < 64)
        for (int i = threadIdx.x; i < nb; i += 64) { const int2 v = cnt[i]; c += (unsigned)v.x; g += (unsigned)v.y; }
    if (half < 2) {
        float a[4];
        partial_sums_f32(reinterpret_cast<const float4*>(half ? pb : pa), nb * (kIcpSlots / 4), t, a);
        double* s_seg = half ? s_segB : s_segA;
        const int row = t >> 3, c4 = (t & 7) * 4;
        s_seg[row * 32 + c4 + 0] = (double)a[0]; s_seg[row * 32 + c4 + 1] = (double)a[1];
        s_seg[row * 32 + c4 + 2] = (double)a[2]; s_seg[row * 32 + c4 + 3] = (double)a[3];
    }
    if (threadIdx.x < 64) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { c += (unsigned)__shfl_xor((int)c, o, 64); g += (unsigned)__shfl_xor((int)g, o, 64); }
        if (threadIdx.x == 0) { s_cnt[0] = (int)c; s_cnt[1] = (int)g; }
    }
    __syncthreads();
    if (t < 128 && half < 2) reduce_rows(half ? s_segB : s_segA, half ? s_sysB : s_sysA, t);
    __syncthreads();
}

// Sum of 29 (padded to 32) accumulators over the 64 lanes of a wavefront by recursive halving: at step s each lane
// keeps the half of its remaining values selected by bit s of its lane id and hands the other half to lane ^ (1 << s),
// so 16 + 8 + 4 + 2 + 1 + 1 = 32 cross-lane moves do what 29 x 6 = 174 full-width reductions did (measured: the
// 174-DPP form cost ~2.2k cycles per wavefront and dominated the launch at 4 wavefronts per SIMD).
// On return lane l holds the wave total of component bitrev5(l & 31) in v[0] (components >= 29 are zero padding).
__device__ __forceinline__ int icp_component_of_lane(int lane) {
    const int l = lane & 31;
    return ((l & 1) << 4) | ((l & 2) << 2) | (l & 4) | ((l & 8) >> 2) | ((l & 16) >> 4);
}
// bitwise select (one v_bfi_b32): written on the bit patterns so that the compiler cannot turn "cond ? v[a] : v[b]" into
// a dynamically indexed register array (which it lowers to a 32-deep compare/select chain per access).
__device__ __forceinline__ float bitsel(unsigned mask, float a, float b) {
    return __uint_as_float((__float_as_uint(a) & mask) | (__float_as_uint(b) & ~mask));
}
// Cross-lane fetch "value of lane (lane ^ kXor)".  xor 1 / 2 are quad permutes, xor 8 a 16-lane row rotation, xor 4 two row
// rotations and a select -- all DPP modifiers on VALU instructions (no LDS crossbar traffic); only xor 16 / 32 cross a DPP row
// and go through ds_bpermute.  30 of the 32 exchanges of the halving tree are xor 1..8: with every exchange on the
// bpermute path the tree cost ~5 k cycles per launch at 16 wavefronts per CU (the crossbar serialises them).
template <int kXor>
__device__ __forceinline__ float lane_xor(float v, int lane) {
    const int iv = __float_as_int(v);
    if constexpr (kXor == 1) return __int_as_float(__builtin_amdgcn_update_dpp(0, iv, 0xB1, 0xf, 0xf, false));   // quad_perm:[1,0,3,2]
    else if constexpr (kXor == 2) return __int_as_float(__builtin_amdgcn_update_dpp(0, iv, 0x4E, 0xf, 0xf, false));   // quad_perm:[2,3,0,1]
    else if constexpr (kXor == 4) {
        const int dn = __builtin_amdgcn_update_dpp(0, iv, 0x124, 0xf, 0xf, false);   // row_ror:4  -> lane i reads i - 4 (mod 16)
        const int up = __builtin_amdgcn_update_dpp(0, iv, 0x12C, 0xf, 0xf, false);   // row_ror:12 -> lane i reads i + 4 (mod 16)
        return __int_as_float((lane & 4) ? dn : up);
    } else if constexpr (kXor == 8) return __int_as_float(__builtin_amdgcn_update_dpp(0, iv, 0x128, 0xf, 0xf, false));   // row_ror:8
    else return __shfl_xor(v, kXor, 64);
}

template <int kStep>
__device__ __forceinline__ void halving_step(float (&v)[32], int lane) {
    constexpr int half = 16 >> kStep;
    const unsigned up = ((lane >> kStep) & 1) ? 0xFFFFFFFFu : 0u;
#pragma unroll
    for (int k = 0; k < half; ++k) {
        const float send = bitsel(up, v[k], v[k + half]);
        const float keep = bitsel(up, v[k + half], v[k]);
        v[k] = keep + lane_xor<(1 << kStep)>(send, lane);
    }
}

__device__ __forceinline__ float wave_sum32_halving(float (&v)[32]) {
    const int lane = threadIdx.x & 63;
    halving_step<0>(v, lane);
    halving_step<1>(v, lane);
    halving_step<2>(v, lane);
    halving_step<3>(v, lane);
    halving_step<4>(v, lane);
    return v[0] + __shfl_xor(v[0], 32, 64);
}

// Sum of the 29 accumulators over ALL kT threads of a workgroup through LDS, in a fixed order: lane pairs first (one DPP add per
// accumulator), even lanes store column-wise [component][kT / 2] (consecutive lanes -> consecutive banks), then component c is
// summed by G = kT / 32 neighbouring threads (16 values each, read as four conflict-free float4 rows) and a G-lane DPP butterfly.
// ~85 instructions per wavefront and 60 KB of LDS traffic per 512-thread workgroup against ~300 instructions per wavefront for
// the register halving tree above (which stays for the RGB-D kernels): the tree was 2.4 k of the 15 k cycles of a level-0 launch.
// out: the workgroup's 32-float partial (components >= 29 are written as zeros).
template <int kT>
__device__ __forceinline__ void block_sum29_lds(const float (&acc)[32], float* s_red /*[29][kT / 2]*/, float* __restrict__ out) {
    constexpr int kHalf = kT / 2, G = kT / 32;
    static_assert(G == 8 || G == 16, "kT must be 256 or 512");
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int c = 0; c < 29; ++c) {
        const float v = acc[c] + lane_xor<1>(acc[c], lane);
        if ((lane & 1) == 0) s_red[c * kHalf + (tid >> 1)] = v;
    }
    __syncthreads();
    const int c = tid / G, g = tid % G;
    float s = 0.f;
    if (c < 29) {
        const float4* __restrict__ row = reinterpret_cast<const float4*>(s_red + c * kHalf);
        float4 v[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) v[m] = row[m * G + g];
#pragma unroll
        for (int m = 0; m < 4; ++m) s += (v[m].x + v[m].y) + (v[m].z + v[m].w);
    }
    s += lane_xor<1>(s, lane);
    s += lane_xor<2>(s, lane);
    s += lane_xor<4>(s, lane);
    if (G == 16) s += lane_xor<8>(s, lane);
    if (g == 0) out[c] = s;
}

// Sum of nb int2 records by the first wavefront; result broadcast through LDS (s_cnt[2]).  int32 wrap-around like the
// reference's int2 sums (reduce.cu:716-772).
__device__ __forceinline__ void reduce_counts(const int2* __restrict__ cnt, int nb, int* s_cnt) {
    if (threadIdx.x < 64) {
        unsigned c = 0, g = 0;
        for (int i = threadIdx.x; i < nb; i += 64) { const int2 v = cnt[i]; c += (unsigned)v.x; g += (unsigned)v.y; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { c += (unsigned)__shfl_xor((int)c, o, 64); g += (unsigned)__shfl_xor((int)g, o, 64); }
        if (threadIdx.x == 0) { s_cnt[0] = (int)c; s_cnt[1] = (int)g; }
    }
    __syncthreads();
}

// Gauss-Newton trace of a tracking step (debug tap "gn_trace", tests/test_gpu_parity_long.py): row r = [0..31] the reduced system of iteration r
// as the device summed it (fp64: 27 packed products, sum r^2, inliers), [32..47] resultRt, [48..56] Rcurr, [57..59] tcurr as iteration r USED
// them; row n_iterations holds the state after the last update.  Written by lanes u = 0..59 of whoever finishes an iteration.
__device__ __forceinline__ void gn_trace_write(double* __restrict__ trace, int it, bool have_sys, const double* s_sys, const GNState* s_st, int u) {
    if (!trace || u < 0) return;
    if (u < 32) { if (have_sys) trace[kGnTraceRow * (it - 1) + u] = s_sys[u]; }
    else if (u < 48) trace[kGnTraceRow * it + u] = s_st->resultRt[u - 32];
    else if (u < 57) trace[kGnTraceRow * it + u] = (double)s_st->Rcurr[u - 48];
    else if (u < 60) trace[kGnTraceRow * it + u] = (double)s_st->tcurr[u - 57];
}

// Correspondence search for one pixel, split in two so that the gathers of all four pixels of a thread are in flight
// together (a per-pixel search-then-accumulate serialises four dependent L2 round trips: ~2 us per launch).
struct IcpCorr { float3 vcurr_g, vcurr_cp, ncurr_g; int j; bool ok; };

// Per-pixel arithmetic of the ICP kernels, every operation rounded on its own and in the order of the CPU restatement the
// parity tests check against (its m33_mul / f3_dot / f3_cross: a plain reading of Core/Cuda/reduce.cu:292-415), contraction off.  Two reasons:
//  * everything that DECIDES something -- the rounded projection (ux, uy), the 0.10 m distance gate, the sin 20 degrees gate, the
//    NaN tests -- is then bit-identical to the oracle, so the inlier set (not just its size) matches by construction, and the
//    seven row entries of every inlier do too; only the accumulation of the 28 products differs (fp32 block sums here, double there)
//    -- held on inputs that sit ON each decision, through every kernel that inlines these functions, by tests/test_gpu_gn_gates.py;
//  * k_icp_iter<512>, k_icp_iter<256>, k_icp_batch_pixels and k_rgbd_iter are separate functions, and left to itself the compiler
//    contracts a * b + c differently in each.  The 1e-7 relative spread that causes is invisible for a room-sized model, but a freshly
//    spawned object (2 000 pixels on two box faces: a 6x6 system with condition ~1e5) turns it into millimetres of pose: the batched
//    loop and the model-by-model loop must agree pixel for pixel (tests/test_gpu_multimodel.py::test_batched_tracking_...).
// Cost: ~20 instructions per pixel (3 mul + 2 add instead of 1 mul + 2 fma per matrix row).
__device__ __forceinline__ float3 icp_mul33(const float* R, float3 v) {
#pragma clang fp contract(off)
    return f3(R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z, R[6] * v.x + R[7] * v.y + R[8] * v.z);
}
__device__ __forceinline__ float icp_dot3(float3 a, float3 b) {
#pragma clang fp contract(off)
    return a.x * b.x + a.y * b.y + a.z * b.z;
}
__device__ __forceinline__ float3 icp_cross3(float3 a, float3 b) {
#pragma clang fp contract(off)
    return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

template <class Args>
__device__ __forceinline__ IcpCorr icp_project(float vx, float vy, float vz, float nx, float ny, float nz, const float* Rc,
                                               float3 tc, const float* Rpi, float3 tp, const Args& a) {
#pragma clang fp contract(off)
    // search(), first half: Core/Cuda/reduce.cu:292-314
    IcpCorr c;
    const float3 g = icp_mul33(Rc, f3(vx, vy, vz));
    c.vcurr_g = f3(g.x + tc.x, g.y + tc.y, g.z + tc.z);
    c.vcurr_cp = icp_mul33(Rpi, f3(c.vcurr_g.x - tp.x, c.vcurr_g.y - tp.y, c.vcurr_g.z - tp.z));
    const int ux = __float2int_rn((c.vcurr_cp.x * a.k.fx) / c.vcurr_cp.z + a.k.cx);
    const int uy = __float2int_rn((c.vcurr_cp.y * a.k.fy) / c.vcurr_cp.z + a.k.cy);
    c.ok = !(ux < 0 || uy < 0 || ux >= a.W || uy >= a.H || c.vcurr_cp.z < 0) && !isnan(nx);
    c.j = c.ok ? uy * a.W + ux : 0;
    c.ncurr_g = icp_mul33(Rc, f3(nx, ny, nz));
    return c;
}

template <class Args>
__device__ __forceinline__ void icp_accumulate(const IcpCorr& c, float3 vprev_g, float3 nprev_g, const float* Rpi, float3 tp,
                                               const Args& a, float* acc) {
#pragma clang fp contract(off)
    // search(), second half + getProducts(): Core/Cuda/reduce.cu:326-415
    // dist = |vprev_g - vcurr_g| <= distThres and sine = |ncurr_g x nprev_g| < angleThres, decided on the squares: sqrtf is monotonic and
    // correctly rounded, so sqrtf(x) <= T  <=>  x <= max{y : sqrtf(y) <= T}, and sqrtf(x) < T  <=>  x < min{y : sqrtf(y) >= T}; the host finds
    // the two boundary floats once (icp_gates) and the kernel saves two IEEE square roots (~30 instructions) per pixel -- same inlier set, bit for bit.
    const float3 dv = f3(vprev_g.x - c.vcurr_g.x, vprev_g.y - c.vcurr_g.y, vprev_g.z - c.vcurr_g.z);
    const float dist2 = icp_dot3(dv, dv);
    const float3 cr = icp_cross3(c.ncurr_g, nprev_g);
    const float sine2 = icp_dot3(cr, cr);
    const bool found = c.ok && sine2 < a.sine2Min && dist2 <= a.dist2Max && !isnan(nprev_g.x);
    if (!found) return;
    const float3 s_cp = c.vcurr_cp;
    const float3 d_cp = icp_mul33(Rpi, f3(vprev_g.x - tp.x, vprev_g.y - tp.y, vprev_g.z - tp.z));
    const float3 n_cp = icp_mul33(Rpi, nprev_g);
    const float3 sxn = icp_cross3(s_cp, n_cp);
    const float row[7] = {n_cp.x, n_cp.y, n_cp.z, sxn.x, sxn.y, sxn.z,
                          icp_dot3(n_cp, f3(s_cp.x - d_cp.x, s_cp.y - d_cp.y, s_cp.z - d_cp.z))};
    int k = 0;
#pragma unroll
    for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int cc = r; cc < 7; ++cc) { acc[k] = fmaf(row[r], row[cc], acc[k]); ++k; }
    acc[28] += 1.0f;
}

__device__ __forceinline__ void seed_state(const PoseDev& pose, GNState& s) {
    for (int k = 0; k < 16; ++k) s.resultRt[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int k = 0; k < 9; ++k) { s.Rprev[k] = pose.R[k]; s.Rcurr[k] = pose.R[k]; s.trR[k] = (k % 4 == 0) ? 1.f : 0.f; }
    for (int k = 0; k < 3; ++k) { s.tprev[k] = pose.t[k]; s.tcurr[k] = pose.t[k]; s.trt[k] = 0.f; }
    m33_inverse_f(s.Rprev, s.Rprev_inv);  // RGBDOdometry.cpp:332
    s.lastICPError = 0.f; s.lastICPCount = 0.f; s.valid = 0;
    s.levelDone = -1; s.lastRGBError = 3.4028234664e38f; s.lastRGBCount = 0.f; s.ill = 0;
}

// ---- The parts of a step.  None of them holds arithmetic of its own: they order the functions above. ----
// First launch of a tracking step, one thread (RGBDOdometry.cpp:239-243,332-344): Rprev = Rcurr = pose, resultRt = I or the SO(3) pre-alignment's rotation
__device__ __forceinline__ void gn_seed(const PoseDev& pose, const So3Result* so3_or_null, GNState& s) {
    seed_state(pose, s);
    for (int k = 0; so3_or_null && k < 9; ++k) s.resultRt[(k / 3) * 4 + k % 3] = so3_or_null->R[k];
}

// Every other launch: the state comes through LDS with one coalesced load (one thread would chase ~80 dependent scalar loads after the solve);
// the caller's next barrier publishes it
__device__ __forceinline__ void gn_stage(GNState* s_st, const GNState* src) {
    if (threadIdx.x < sizeof(GNState) / 4) reinterpret_cast<uint32_t*>(s_st)[threadIdx.x] = reinterpret_cast<const uint32_t*>(src)[threadIdx.x];
}

// What ONE workgroup of a launch leaves for the next launch and the finalize step, behind the barrier that follows the update: the state (84 words),
// the reduced system just solved (32 floats) and the trace row -- one store instruction each, on lanes of their own.
__device__ __forceinline__ void gn_publish(GNState* st_out, float* log_or_null, double* trace_or_null, int it, bool have_sys, const double* s_sys,
                                           const GNState* s_st) {
    constexpr int kWords = (int)(sizeof(GNState) / 4), kMinThreads = 256;   // the smallest workgroup that publishes
    static_assert(kWords + 32 <= kMinThreads, "state + log lanes");
    static_assert(kWords + 32 + 60 <= kMinThreads, "trace lanes");
    const int tid = threadIdx.x;
    if (tid < kWords) reinterpret_cast<uint32_t*>(st_out)[tid] = reinterpret_cast<const uint32_t*>(s_st)[tid];
    else if (tid < kWords + 32 && log_or_null && have_sys) log_or_null[tid - kWords] = (float)s_sys[tid - kWords];
    gn_trace_write(trace_or_null, it, have_sys, s_sys, s_st, tid - (kWords + 32));
}

// The pixel phase of one round of kPx slots per thread: all projections, then all gathers (independent loads in flight together: a per-pixel
// search-then-accumulate serialises kPx dependent L2 round trips), then the products.  act: the slot's pixel lies inside the workgroup's chunk (a
// masked slot re-read a valid pixel and adds nothing); won: the slot is live for the wavefront (a scalar branch skips it otherwise).
struct IcpPx { float vx, vy, vz, nx, ny, nz; };   // one streamed pixel of the frame's vertex / normal maps
template <int kPx, class Args>
__device__ __forceinline__ void icp_slots(const IcpPx (&px)[kPx], const bool (&act)[kPx], const bool (&won)[kPx], const float* vp, const float* np, int P,
                                          const float* Rc, float3 tc, const float* Rpi, float3 tp, const Args& a, float* acc) {
    IcpCorr cor[kPx];
    float3 pv[kPx], pn[kPx];
#pragma unroll
    for (int q = 0; q < kPx; ++q) {
        if (!won[q]) continue;
        cor[q] = icp_project(px[q].vx, px[q].vy, px[q].vz, px[q].nx, px[q].ny, px[q].nz, Rc, tc, Rpi, tp, a);
        cor[q].ok = cor[q].ok && act[q];
        cor[q].j = cor[q].ok ? cor[q].j : 0;
    }
#pragma unroll
    for (int q = 0; q < kPx; ++q) {
        if (!won[q]) continue;
        const int j = cor[q].j;
        pv[q] = f3(vp[j], vp[P + j], vp[2 * P + j]);
        pn[q] = f3(np[j], np[P + j], np[2 * P + j]);
    }
#pragma unroll
    for (int q = 0; q < kPx; ++q)
        if (won[q]) icp_accumulate(cor[q], pv[q], pn[q], Rpi, tp, a, acc);
}

// The workgroup's 32-float partial, out[blockIdx.x][32], from the wavefronts' sums s_part[kT / 64][32] (wave_sum32_halving; components >= 29 are
// written as zeros)
template <int kT>
__device__ __forceinline__ void store_block_partial(const float* s_part, float* out) {
    const int tid = threadIdx.x;
    if (tid < kIcpSlots) {
        float sv = 0.f;
        if (tid < 29) {
#pragma unroll
            for (int w = 0; w < kT / 64; ++w) sv += s_part[w * kIcpSlots + tid];
        }
        out[blockIdx.x * kIcpSlots + tid] = sv;
    }
}

// End of a tracking step, one thread: Model::pose / lastPose / statistics from the final state (RGBDOdometry.cpp:476-496, Model.cpp:437-446) and the
// object-model jump rule.  photometric: the step had the RGB term -- an increment beyond 0.3 m is reverted (RGBDOdometry.cpp:477-481) and the RGB
// statistics are the state's; without it they read 0 and nothing is rejected.
__device__ __forceinline__ void pose_from_state(const GNState& st, const So3Result* so3, float jump_limit, bool photometric, PoseDev& p) {
    const float dx = st.tcurr[0] - st.tprev[0], dy = st.tcurr[1] - st.tprev[1], dz = st.tcurr[2] - st.tprev[2];
    const bool rejected = photometric && (double)sqrtf(dx * dx + dy * dy + dz * dz) > 0.3;
    for (int k = 0; k < 9; ++k) { p.lastR[k] = st.Rprev[k]; p.R[k] = rejected ? st.Rprev[k] : st.Rcurr[k]; }
    for (int k = 0; k < 3; ++k) { p.lastT[k] = st.tprev[k]; p.t[k] = rejected ? st.tprev[k] : st.tcurr[k]; }
    p.lastICPError = st.lastICPError; p.lastICPCount = st.lastICPCount;
    p.rejected = rejected ? 1 : 0;
    p.lastRGBError = photometric ? st.lastRGBError : 0.f; p.lastRGBCount = photometric ? st.lastRGBCount : 0.f;
    if (so3) { p.lastSO3Error = so3->error; p.lastSO3Count = so3->count; p.so3Iterations = so3->iterations; }
    else { p.lastSO3Error = 0.f; p.lastSO3Count = 0.f; p.so3Iterations = 0; }
    const float3 trt = rejected ? f3(0.f, 0.f, 0.f) : f3(st.trt[0], st.trt[1], st.trt[2]);
    p.incT[0] = trt.x; p.incT[1] = trt.y; p.incT[2] = trt.z;
    p.illIterations = st.ill;   // (the photometric loop does not count: its combined system goes through the wave Gauss-Jordan)
    if (jump_limit > 0.f && norm3(trt) >= jump_limit) p.alive = 0;   // `float d > 0.2` is a DOUBLE comparison upstream (MaskFusion.cpp:268): true from 0.2f on
    pose_derive(p);
}

}  // namespace mf
