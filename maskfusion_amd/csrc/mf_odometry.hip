// mf_odometry.hip -- frame-to-model projective ICP with the whole Gauss-Newton loop resident on the device.
//
// Replaces (paths in the reference's tree; initICPModel, the model-side pyramid, is mf_model_pyramid.hip):
//   icpStep / ICPReduction / reduceSum    Core/Cuda/reduce.cu:92-187,259-525
//   the host side of getIncrementalTransformation (LDLT, SE(3) update)  RGBDOdometry.cpp:327-497,
//                                         Core/Utils/OdometryProvider.h:32-90
//
// Design (MI355X): the reference runs 19 x {kernel, reduce kernel, sync, D2H, host LDLT} per model per frame.
// Here one launch per iteration does everything: its prologue reduces the previous launch's per-workgroup
// partial sums in a fixed order, solves the 6x6 system in fp64 and updates the pose (every workgroup does this
// redundantly and identically, so no workgroup ever waits on another inside a launch -- visibility comes from
// the kernel boundary only), then streams the current vertex/normal planes, gathers the model planes, and reduces 29
// accumulators through LDS (lane pairs by DPP, column-wise stores, 16-lane butterflies).  No host round trip, no atomics,
// bit-reproducible run to run.  With the photometric term an iteration is two launches (k_rgbd_iter, k_rgb_step).
// A launch per iteration is the cheapest device-wide synchronisation this GPU offers: the same loop inside one persistent
// launch (device-wide barriers) was measured 5.8x slower in round 3 and removed.
// This file holds the solve (ldlt6_solve ... gn_finish_wg, gn_step_wg: the test builds cut it out of this file's text), the kernels of the three
// loops, their argument structs and launch forms; the reductions, the per-pixel arithmetic and the other parts the loops share are mf_gn_device.h.
#include <string.h>

#include "mf_internal.h"
#include "mf_device.h"
#include "mf_rgbd_device.h"
#include "mf_gn_device.h"

namespace mf {

// ------------------------------------------------------------------------------------------------
// small fp64 / fp32 linear algebra for the per-iteration solve (single thread)
// ------------------------------------------------------------------------------------------------
// LDL^T in double, fully unrolled so that the 6x6 system lives in registers (a dynamically indexed local array would be
// spilled to scratch memory and turn this ~200-flop solve into ~40 us of dependent scratch round trips).  Stands in for
// Eigen::LDLT (RGBDOdometry.cpp:451-459); Eigen pivots on the diagonal, which for these symmetric positive definite
// systems changes the result only by rounding.  A non-positive / vanishing pivot zeroes that component (Eigen's
// behaviour for singular systems) instead of dividing by it.
__device__ __forceinline__ void ldlt6_solve(double (&A)[6][6], const double (&b)[6], double (&x)[6], double* min_pivot_ratio = nullptr) {
    double maxdiag = 0.0, minpiv = 1.7976931348623157e308;
#pragma unroll
    for (int i = 0; i < 6; ++i) maxdiag = fmax(maxdiag, fabs(A[i][i]));
    const double tol = maxdiag * 1e-14;
    double dinv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double d = A[k][k];
        const bool ok = d > tol;
        minpiv = fmin(minpiv, ok ? d : 0.0);
        dinv[k] = ok ? rcp_d(d) : 0.0;   // v_rcp_f64 + Newton: an IEEE division is a ~40-instruction dependent chain per pivot
        // the lower triangle (i >= j) is the working copy; col = column k of the current Schur complement
        double col[6];
#pragma unroll
        for (int i = k + 1; i < 6; ++i) col[i] = A[i][k];
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const double l = col[i] * dinv[k];
#pragma unroll
            for (int j = k + 1; j <= i; ++j) A[i][j] -= l * col[j];
            A[i][k] = l;  // L below the diagonal
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
#pragma unroll
        for (int j = 0; j < i; ++j) s -= A[i][j] * y[j];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] *= dinv[i];
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int j = i + 1; j < 6; ++j) s -= A[j][i] * x[j];
        x[i] = s;
    }
    // smallest pivot over largest diagonal entry: >= 1 / cond(A) for a positive definite A (0 when a pivot vanished or A = 0)
    if (min_pivot_ratio) *min_pivot_ratio = maxdiag > 0.0 ? minpiv / maxdiag : 0.0;
}

// Wave-parallel 6x6 solve: Gauss-Jordan on the augmented [A|b] with one lane per element (lanes 0..41 of one
// wavefront, fp64, no pivoting -- the systems are symmetric positive definite; a vanishing pivot zeroes that component
// like Eigen::LDLT::solve does for singular systems).  Six rank-1 steps of {3 shuffles, 1 fma} replace a ~3 us
// single-thread LDL^T; the serial ldlt6_solve above is kept as the executable specification (tests compare both).
// sys: 27 packed upper-triangle products of the 7-vector row (reduce.cu:378-411 order) in LDS.  Returns x in every lane.
__device__ __forceinline__ int solve6_lane_index(int& r, int& c) {
    const int l = threadIdx.x & 63;
    r = l < 42 ? l / 7 : 0; c = l < 42 ? l % 7 : 0;
    const int i = r < c ? r : c, j = r < c ? c : r;                 // A is symmetric; column 6 is b
    return (c == 6) ? (r * 7 - (r * (r - 1)) / 2 + (6 - r)) : (i * 7 - (i * (i - 1)) / 2 + (j - i));
}
__device__ __forceinline__ void solve6_wave_core(double v, int r, int c, double (&x)[6]) {
    double maxdiag = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) maxdiag = fmax(maxdiag, fabs(__shfl(v, k * 8, 64)));
    const double tol = maxdiag * 1e-14;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double pivot = __shfl(v, k * 8, 64);
        const double rowk = __shfl(v, k * 7 + c, 64);
        const double colk = __shfl(v, r * 7 + k, 64);
        const double inv = pivot > tol ? rcp_d(pivot) : 0.0;
        const double scaled = rowk * inv;
        v = (r == k) ? scaled : v - colk * scaled;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = __shfl(v, k * 7 + 6, 64);
}
__device__ __forceinline__ void solve6_wave(const double* sys, double (&x)[6]) {
    int r, c;
    const int idx = solve6_lane_index(r, c);
    const double v = (double)(float)sys[idx];                        // the reference hands float A/b to the host
    solve6_wave_core(v, r, c, x);
}
// lastA = A_rgbd + w^2 A_icp, lastb = b_rgbd + w b_icp (RGBDOdometry.cpp:447-452; sic -- the ICP step is scaled by 1/w)
__device__ __forceinline__ void solve6_wave_rgbd(const double* sysIcp, const double* sysRgb, double wA, double wb, double (&x)[6]) {
    int r, c;
    const int idx = solve6_lane_index(r, c);
    const double v = (double)(float)sysRgb[idx] + ((c == 6) ? wb : wA) * (double)(float)sysIcp[idx];
    solve6_wave_core(v, r, c, x);
}

// Pose update from the Gauss-Newton step x: RGBDOdometry.cpp:428-474 (icp && !rgb branch) +
// OdometryProvider::computeUpdateSE3.  Everything is unrolled with compile-time indices (registers only).
__device__ __forceinline__ void gn_update_from_x(const double (&x)[6], float res, float inl, const GNState& in, GNState& out) {
    out.lastICPError = sqrtf(res) / inl;
    out.lastICPCount = inl;
    // resultRt <- [exp(w) | t] * resultRt
    double Rw[3][3];
    rodrigues_d(x[3], x[4], x[5], Rw);
    double nr[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            nr[r][c] = Rw[r][0] * in.resultRt[0 * 4 + c] + Rw[r][1] * in.resultRt[1 * 4 + c] + Rw[r][2] * in.resultRt[2 * 4 + c] +
                       x[r] * in.resultRt[3 * 4 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) out.resultRt[r * 4 + c] = nr[r][c];
#pragma unroll
    for (int c = 0; c < 4; ++c) out.resultRt[12 + c] = in.resultRt[12 + c];
    float trR[9], trt[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) trR[r * 3 + c] = (float)nr[r][c];
        trt[r] = (float)nr[r][3];
    }
    // currentT = [Rprev|tprev] * transform.inverse()
    float iR[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) iR[r * 3 + c] = trR[c * 3 + r];
    const float3 itv = mul33(iR, f3(trt[0], trt[1], trt[2]));
    const float it3[3] = {-itv.x, -itv.y, -itv.z};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out.Rcurr[r * 3 + c] = in.Rprev[r * 3 + 0] * iR[0 * 3 + c] + in.Rprev[r * 3 + 1] * iR[1 * 3 + c] +
                                   in.Rprev[r * 3 + 2] * iR[2 * 3 + c];
    const float3 tv = mul33(in.Rprev, f3(it3[0], it3[1], it3[2]));
    out.tcurr[0] = tv.x + in.tprev[0]; out.tcurr[1] = tv.y + in.tprev[1]; out.tcurr[2] = tv.z + in.tprev[2];
#pragma unroll
    for (int k = 0; k < 9; ++k) { out.Rprev[k] = in.Rprev[k]; out.Rprev_inv[k] = in.Rprev_inv[k]; out.trR[k] = trR[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { out.tprev[k] = in.tprev[k]; out.trt[k] = trt[k]; }
    out.valid = 1;
    out.levelDone = in.levelDone; out.lastRGBError = in.lastRGBError; out.lastRGBCount = in.lastRGBCount; out.ill = in.ill;
}

// Serial form (one thread): unpack -> LDL^T -> update.  mf_k_gn_solve (tests/test_gpu_kernels.py) runs it next to the wave solver
// and the oracle's restatement of Eigen's LDLT / OdometryProvider::rodrigues / computeUpdateSE3.
__device__ __forceinline__ void gn_solve_update_serial(const double* sys, const GNState& in, GNState& out) {
    double A[6][6], b[6], x[6];
    int shift = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 7; ++j) {
            // (the reference rounds A, b to fp32 on their way to the host; the fp32 per-workgroup partials already differ from
            // an all-fp64 sum by ~1e-7 relative, so the extra rounding -- 54 quarter-rate conversions on this single
            // thread -- is dropped)
            const double value = sys[shift++];
            if (j == 6) b[i] = value;
            else { A[i][j] = value; A[j][i] = value; }
        }
    ldlt6_solve(A, b, x);
    gn_update_from_x(x, (float)sys[27], (float)sys[28], in, out);
}

// The same update with the state resident in LDS, run by WAVEFRONT 0 ALONE (the other wavefronts of the workgroup return at once and wait
// at the caller's next barrier, as they always did).  Lanes 0..11 each solve the system redundantly in registers (so x needs no broadcast:
// the LDL^T is ~120 instructions whichever way it is cut) and compute ONE entry of the 3x4 block of resultRt; the float work after that --
// transform^-1, Rcurr = Rprev iR, tcurr = Rprev it + tprev -- is exchanged between those lanes with wavefront shuffles.
// Round 3 exchanged through LDS behind three workgroup barriers: the in-kernel stamps of round 4 (profiles/r04a_icp_prof.txt) priced those
// three steps at 500 + 650 + 480 of the prologue's ~4 000 cycles, more than the LDL^T (1 000) or exp + composition (1 000).  LDS
// instructions of ONE wavefront execute in issue order, so reading the old resultRt and then overwriting it needs no barrier either.
// The float expressions are those of the CPU restatement, operation by operation (contraction off): given the same T the pose is the
// oracle's bit for bit, in every kernel that calls this.
// s_st is updated in place: resultRt, Rcurr, tcurr, trR, trt, lastICPError / Count, valid, ill; everything else keeps its value.  s_pose
// receives Rcurr[9] tcurr[3] (slots 0..11; slots 12..23 = Rprev_inv, tprev are pose-independent and written by the caller once).
// The caller places a barrier between this call and any other wavefront's use of s_st / s_pose.
// Shader-clock stamps inside the solve ("icpProfile").  `on` is set in the one thread that keeps them (thread 0 of workgroup 0): a flag beside the
// stamps, not a null pointer in the other threads, so that the struct stays in registers
struct GnStamps { unsigned long long t[6]; bool on; };
__device__ __forceinline__ void gn_finish_wg(const double* s_sys, GNState* s_st, float* s_pose /*[24]*/, GnStamps* stamps = nullptr) {
    const bool stamped = stamps != nullptr && stamps->on;
    if (threadIdx.x == 64) {   // wavefront 1 has nothing to do until the caller's barrier: the iteration's statistics (an IEEE square root and a
                               // division, ~150 cycles) leave wavefront 0's chain
        const float res = (float)s_sys[27], inl = (float)s_sys[28];
        s_st->lastICPError = sqrtf(res) / inl;
        s_st->lastICPCount = inl;
        s_st->valid = 1;
    }
    if (threadIdx.x >= 64) return;
    const int l = threadIdx.x;
    const int r = (l >> 2) & 3, c = l & 3;   // lanes 0..11: entry (r, c) of the 3x4 block
    // pose-independent operands of the float tail, fetched before the solve (their latency hides under it): row `row` of Rprev, tprev[q]
    const int rr = l / 3, cc = l - 3 * rr, q = l - 9;
    const bool isR = l < 9, isT = l >= 9 && l < 12;
    const int row = isR ? rr : (isT ? q : 0);
    const float p0 = s_st->Rprev[row * 3 + 0], p1 = s_st->Rprev[row * 3 + 1], p2 = s_st->Rprev[row * 3 + 2];
    const float tpq = s_st->tprev[isT ? q : 0];
    double nr = 0.0;
    int ill = 0;
    if (l < 12) {
        double A[6][6], b[6], x[6], ratio;
        int shift = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 7; ++j) {
                const double value = s_sys[shift++];
                if (j == 6) b[i] = value;
                else { A[i][j] = value; A[j][i] = value; }
            }
        if (stamped) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); stamps->t[0] = __builtin_amdgcn_s_memtime(); }
        ldlt6_solve(A, b, x, &ratio);
        ill = (s_sys[28] < 6.0 || !(ratio >= 1e-8)) ? 1 : 0;   // outside the stated domain of this solver (finding F4): counted, see GNState::ill
        if (stamped) stamps->t[1] = __builtin_amdgcn_s_memtime() + (unsigned long long)(x[0] == 1.2345e300);   // (the stamp waits for the solve)
        double Rw[3][3];
        rodrigues_d(x[3], x[4], x[5], Rw);
        const double w0 = r == 0 ? Rw[0][0] : (r == 1 ? Rw[1][0] : Rw[2][0]);
        const double w1 = r == 0 ? Rw[0][1] : (r == 1 ? Rw[1][1] : Rw[2][1]);
        const double w2 = r == 0 ? Rw[0][2] : (r == 1 ? Rw[1][2] : Rw[2][2]);
        const double xr = r == 0 ? x[0] : (r == 1 ? x[1] : x[2]);
        const double* Rt = s_st->resultRt;
        nr = w0 * Rt[0 * 4 + c] + w1 * Rt[1 * 4 + c] + w2 * Rt[2 * 4 + c] + xr * Rt[3 * 4 + c];   // resultRt <- [exp(w) | t] * resultRt
        if (stamped) stamps->t[2] = __builtin_amdgcn_s_memtime() + (unsigned long long)(nr == 1.2345e300);
    }
    // Isometry3f transform T = float(resultRt[0..2][0..3]) lives in lanes r * 4 + c; currentT = [Rprev|tprev] * transform.inverse():
    // iR = trR^T, it = -iR trt, Rcurr = Rprev iR, tcurr = Rprev it + tprev.  The twelve entries are broadcast with v_readlane (a scalar
    // register each, a few cycles) and every lane selects its operands: no LDS round trip, no ds_bpermute latency on the chain.
    const float tv = (float)nr;
    const int tvb = __float_as_int(tv);
    float T[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) T[j] = __int_as_float(__builtin_amdgcn_readlane(tvb, j));
    // lanes 0..8: a_k = T[cc][k]; lanes 9..11: a_k = T[k][q]
    const float a0 = isR ? (cc == 0 ? T[0] : (cc == 1 ? T[4] : T[8])) : (q == 0 ? T[0] : (q == 1 ? T[1] : T[2]));
    const float a1 = isR ? (cc == 0 ? T[1] : (cc == 1 ? T[5] : T[9])) : (q == 0 ? T[4] : (q == 1 ? T[5] : T[6]));
    const float a2 = isR ? (cc == 0 ? T[2] : (cc == 1 ? T[6] : T[10])) : (q == 0 ? T[8] : (q == 1 ? T[9] : T[10]));
    const float t0 = T[3], t1 = T[7], t2 = T[11];                                                   // trt
    float rcur, itq;
    {
#pragma clang fp contract(off)
        rcur = p0 * a0 + p1 * a1 + p2 * a2;                 // lanes 0..8: Rcurr[rr][cc] = sum_k Rprev[rr][k] iR[k][cc], iR[k][cc] = T[cc][k]
        itq = -(a0 * t0 + a1 * t1 + a2 * t2);               // lanes 9..11: it[q] = -(iR trt)[q], iR[q][k] = T[k][q]
    }
    const int itb = __float_as_int(itq);
    const float i0 = __int_as_float(__builtin_amdgcn_readlane(itb, 9)), i1 = __int_as_float(__builtin_amdgcn_readlane(itb, 10)),
                i2 = __int_as_float(__builtin_amdgcn_readlane(itb, 11));
    float tcur;
    {
#pragma clang fp contract(off)
        tcur = (p0 * i0 + p1 * i1 + p2 * i2) + tpq;         // lanes 9..11: tcurr[q]
    }
    if (l < 12) {
        s_st->resultRt[r * 4 + c] = nr;   // behind the broadcast: every lane of the wavefront has read the old block by now (one wavefront,
                                          // instructions in order -- and a schedule-independent order for the CPU-executed build)
        if (c < 3) s_st->trR[r * 3 + c] = tv; else s_st->trt[r] = tv;
    }
    if (isR) { s_st->Rcurr[l] = rcur; s_pose[l] = rcur; }
    else if (isT) { s_st->tcurr[q] = tcur; s_pose[9 + q] = tcur; }
    if (l == 0) {
        s_st->ill += ill;
        if (stamped) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); stamps->t[3] = __builtin_amdgcn_s_memtime(); stamps->t[4] = stamps->t[3]; stamps->t[5] = stamps->t[3]; }
    }
}

// Finishing the previous iteration, identically in every workgroup that calls it: its state -> LDS, its per-workgroup partial sums -> s_sys in a
// fixed order, solve + pose update in place (Rcurr / tcurr also to s_pose[0..11]).  The caller places a barrier behind it.
__device__ __forceinline__ void gn_step_wg(const GNState* st_in, const float* __restrict__ partials, int nb, double* s_seg, double* s_sys, GNState* s_st,
                                           float* s_pose) {
    gn_stage(s_st, st_in);
    reduce_partials(partials, nb, s_seg, s_sys);   // (its barriers also publish s_st)
    gn_finish_wg(s_sys, s_st, s_pose);
}

// ------------------------------------------------------------------------------------------------
// The ICP iteration kernel.
// ------------------------------------------------------------------------------------------------
// Boundary floats of the two gates on the squared quantities (see icp_accumulate): d2 = max{y : sqrtf(y) <= distThres},
// s2 = min{y : sqrtf(y) >= angleThres}.  Host libm's sqrtf is correctly rounded, like the device's.
static void icp_gates(float distThres, float angleThres, float& dist2Max, float& sine2Min) {
    float d2 = distThres * distThres;
    while (sqrtf(d2) > distThres) d2 = nextafterf(d2, 0.f);
    while (sqrtf(nextafterf(d2, INFINITY)) <= distThres) d2 = nextafterf(d2, INFINITY);
    float s2 = angleThres * angleThres;
    while (sqrtf(s2) < angleThres) s2 = nextafterf(s2, INFINITY);
    while (s2 > 0.f && sqrtf(nextafterf(s2, 0.f)) >= angleThres) s2 = nextafterf(s2, 0.f);
    dist2Max = d2; sine2Min = s2;
}

struct IcpKArgs {
    const float* vc; const float* nc; const float* vp; const float* np;
    int W, H; Intr k;
    float dist2Max, sine2Min;      // the 0.10 m / sin 20 deg gates of reduce.cu:326-341 on the SQUARED quantities (icp_gates)
    const float* partials_in; int nb_in;
    float* partials_out;
    const GNState* st_in; GNState* st_out;
    float* log_out;
    double* trace; int it;         // optional (parity tests): the model's Gauss-Newton trace (mf_internal.h: kGnTraceRow) and this launch's iteration
    unsigned long long* prof_out;  // optional: 16 shader-clock stamps of workgroup 0 / thread 0 (8 of the launch + 6 inside the solve)
    const PoseDev* pose_in;        // first launch of a tracking step: seed the state from the model pose
    const So3Result* so3_in;       // ... and resultRt's rotation from the SO(3) pre-alignment (RGBDOdometry.cpp:338-344)
};

// Workgroup shape.  Per launch a CU spends its time in three VALU-throughput-bound stretches (one VALU instruction per 4
// cycles per SIMD, 4 SIMDs): the per-pixel chain (project -> gather -> gate -> 29 products, ~250 instructions per 64
// pixels), the 32-value halving reduction (~300 instructions PER WAVEFRONT, however few pixels it carried) and the
// single-wavefront solve.  With 16 wavefronts per CU at one pixel per thread the reduction alone was 16 x 300 x 4 / 4 =
// 4 800 cycles of every launch; 8 wavefronts carrying up to 3 pixels per thread halve that while two wavefronts per SIMD
// plus all gathers of a thread in flight together still hide the gather latency.
constexpr int kIcpThreads = 512;
constexpr int kIcpPx = 3;           // pixel slots per thread (a workgroup's chunk is <= kIcpPx * kIcpThreads pixels)
constexpr int kIcpMaxBlocks = 240;  // <= one workgroup per CU (256 CUs) with a little slack for busy CUs

__host__ __device__ inline int icp_chunk(int P, int nblocks) {
    const int c = (P + nblocks - 1) / nblocks;
    return ((c + 63) / 64) * 64;
}

// kT: threads per workgroup (512 at level 0; 256 at the coarse levels, where there are fewer 512-pixel chunks than CUs:
// twice the workgroups, half the wavefronts per CU -> half the per-CU halving-reduction time)
// kPx: pixel slots per thread = ceil(chunk / kT): 3 at level 0 of a VGA frame (1280-pixel chunks), 2 at level 1 (320), 1 at level 2 (256).
// The pixel phase is VALU-bound (~330 instructions per pixel; a SIMD issues one wave-instruction per 2 cycles), so a slot nobody needs is
// not free: round 3 ran three slots at every level -- at level 2 two thirds of the phase's instructions worked on masked pixels.  A slot
// whose 64 pixels all lie beyond the chunk is skipped by the WHOLE wavefront (a scalar branch, no exec-mask bookkeeping): at level 0 the
// chunk is 2.5 slots, wavefronts 4..7 skip the third one and every SIMD carries 5 slots instead of 6.  Masked or skipped, a slot adds
// nothing to the sums: results are bit-identical to the three-slot form.
template <int kT, int kPx>
__global__ __launch_bounds__(kT) void k_icp_iter(const IcpKArgs a) {
    constexpr bool kSkipIdleSlots = kT == 256 && kPx > 1;
    __shared__ double s_seg[32 * 32];
    __shared__ double s_sys[32];
    __shared__ float s_pose[24];  // Rcurr[9] tcurr[3] Rprev_inv[9] tprev[3]
    __shared__ float s_red[29 * (kT / 2)];
    __shared__ GNState s_st;      // the Gauss-Newton state: loaded (or seeded), updated in place by gn_finish_wg, stored by workgroup 0

    const int tid = threadIdx.x;
    // Every argument the launch reads is requested HERE, as one batch of scalar loads behind one wait.  Left to itself the compiler loads an
    // argument in the block that first uses it: st_in in front of the state's load, the maps and gridDim behind it, the partials' in front of the
    // reduce -- five dependent round trips to the argument buffer, each cold, in a launch that the next one waits for ("Round 14").
    asm volatile("" :: "s"(a.vc), "s"(a.nc), "s"(a.vp), "s"(a.np), "s"(a.W), "s"(a.H), "s"(a.k.fx), "s"(a.k.fy), "s"(a.k.cx), "s"(a.k.cy),
                 "s"(a.dist2Max), "s"(a.sine2Min), "s"(a.partials_in), "s"(a.nb_in), "s"(a.partials_out), "s"(a.st_in), "s"(a.st_out), "s"(a.log_out),
                 "s"(a.trace), "s"(a.it), "s"(a.prof_out), "s"(a.pose_in), "s"(a.so3_in), "s"(gridDim.x));
    if (a.pose_in == nullptr) gn_stage(&s_st, a.st_in);
    else if (tid == 0) gn_seed(*a.pose_in, a.so3_in, s_st);
    const bool prof = a.prof_out != nullptr && blockIdx.x == 0 && tid == 0;
    unsigned long long stamp[8];
    GnStamps gst;
    gst.on = prof;
    if (prof) stamp[0] = __builtin_amdgcn_s_memtime();
    const int P = a.W * a.H;
    // A workgroup owns a contiguous chunk of <= kPx * kT pixels (icp_grid_blocks keeps the grid <= one workgroup
    // per CU so that a launch is ONE round of workgroups: 300 workgroups of 1024 px on 256 CUs ran as two rounds and
    // doubled the level-0 launch time).  Thread t handles pixels beg + t + q * kT, q < kPx.
    const int chunk = icp_chunk(P, gridDim.x);
    const int beg = blockIdx.x * chunk, end = min(P, beg + chunk);

    // (1) issue the pose-independent streamed loads first so their latency overlaps the solve below
    int idx[kPx]; bool act[kPx], won[kPx];
    IcpPx px[kPx];
#pragma unroll
    for (int q = 0; q < kPx; ++q) {
        // lanes past the end of the chunk re-read its last pixel and are masked out of the sums below: no divergent control flow
        // around the loads / projections / gathers (the exec-mask bookkeeping was ~10 % of the pixel phase); a slot that is past
        // the end for the whole wavefront is skipped with a scalar branch
        idx[q] = beg + q * kT + tid;
        act[q] = idx[q] < end;
        // (only where whole wavefronts are known to idle: a scalar branch is a scheduling fence for the loads around it, and at level 0 --
        // every wavefront carries at least two full slots -- the fenced form measured 0.2 us SLOWER per launch, profiles/r04b_*)
        won[q] = kSkipIdleSlots ? (__builtin_amdgcn_readfirstlane(beg + q * kT + (tid & ~63)) < end) : true;
        px[q] = IcpPx{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (won[q]) {
            const int i = min(idx[q], P - 1);
            px[q] = IcpPx{a.vc[i], a.vc[P + i], a.vc[2 * P + i], a.nc[i], a.nc[P + i], a.nc[2 * P + i]};
        }
    }

    // (2) prologue: finish the previous iteration (reduce -> solve -> pose), identically in every workgroup -- gn_step_wg's three calls, with the
    // streamed loads issued in front of them and the stamps between them
    if (prof) stamp[1] = __builtin_amdgcn_s_memtime();
    if (a.nb_in > 0) {
        reduce_partials(a.partials_in, a.nb_in, s_seg, s_sys);   // (its barriers also publish s_st)
        if (prof) stamp[2] = __builtin_amdgcn_s_memtime();
        gn_finish_wg(s_sys, &s_st, s_pose, &gst);   // solve, exp, pose composition: state in place, Rcurr / tcurr -> s_pose[0..11]
    } else {
        __syncthreads();
    }
    if (tid < 12) {   // the pose-independent half of s_pose, and on the first launch of a tracking step the seeded Rcurr / tcurr
        s_pose[12 + tid] = tid < 9 ? s_st.Rprev_inv[tid] : s_st.tprev[tid - 9];
        if (a.nb_in == 0) s_pose[tid] = tid < 9 ? s_st.Rcurr[tid] : s_st.tcurr[tid - 9];
    }
    if (prof) { if (a.nb_in == 0) stamp[2] = stamp[1]; stamp[3] = __builtin_amdgcn_s_memtime(); }
    __syncthreads();
    if (prof) stamp[4] = __builtin_amdgcn_s_memtime();
    if (blockIdx.x == 0) gn_publish(a.st_out, a.log_out, a.trace, a.it, a.nb_in > 0, s_sys, &s_st);

    float Rc[9], Rpi[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Rc[k] = s_pose[k]; Rpi[k] = s_pose[12 + k]; }
    const float3 tc = f3(s_pose[9], s_pose[10], s_pose[11]);
    const float3 tp = f3(s_pose[21], s_pose[22], s_pose[23]);

    // (3) normal equations of this thread's pixel
    float acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.f;
    icp_slots<kPx>(px, act, won, a.vp, a.np, P, Rc, tc, Rpi, tp, a, acc);

    // (4) wavefront reduction (halving tree), one LDS stage across the wavefronts, one 128 B partial per workgroup
    if (prof) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp[5] = __builtin_amdgcn_s_memtime(); }
    block_sum29_lds<kT>(acc, s_red, a.partials_out + blockIdx.x * kIcpSlots);
    if (prof) stamp[6] = __builtin_amdgcn_s_memtime();
    if (prof) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp[7] = __builtin_amdgcn_s_memtime();
#pragma unroll
        for (int k = 0; k < 8; ++k) a.prof_out[k] = stamp[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) a.prof_out[8 + k] = a.nb_in > 0 ? gst.t[k] : 0ull;
    }
}

// threads per workgroup of the ICP-only kernel for an image of P pixels
static int icp_threads_for(int P) { return ((P + kIcpThreads - 1) / kIcpThreads < kIcpMaxBlocks) ? 256 : kIcpThreads; }

static int icp_blocks_capped(int W, int H, int cap256) {
    const int P = W * H;
    const int T = icp_threads_for(P);
    const int cap = T == 256 ? cap256 : kIcpMaxBlocks;
    int nb = (P + T - 1) / T;
    if (nb > cap) {
        nb = cap;
        while (icp_chunk(P, nb) > kIcpPx * T) ++nb;  // larger images: more than one round of workgroups
    }
    return nb;
}
// grid of the RGB-D kernels (512 threads whatever the level) and the upper bound older callers size their scratch with
int icp_grid_blocks(int W, int H) { return icp_blocks_capped(W, H, kIcpMaxBlocks); }
// grid of the geometric kernel k_icp_iter.  A level that runs 256-thread workgroups (fewer than 240 chunks of 512 pixels: levels 1 and 2 of
// a VGA frame) gets one workgroup per 256 pixels up to 320 of them -- level 1: 300 workgroups, ONE pixel slot per thread, two workgroups on
// 44 of the 256 CUs (23 KB of LDS and 4 wavefronts each) -- instead of 240 chunks of 320 pixels whose second slot kept one wavefront in
// four busy and the other three waiting for it (round 4: the pixel phase is VALU-bound, a slot costs what it costs however few lanes use it).
constexpr int kIcpGeoCap256 = 320;
int icp_geo_grid_blocks(int W, int H) { return icp_blocks_capped(W, H, kIcpGeoCap256); }

// pixel slots per thread the launch needs: ceil(chunk / threads), 1..kIcpPx
int icp_pixel_slots(int W, int H) {
    const int P = W * H, T = icp_threads_for(P);
    return (icp_chunk(P, icp_geo_grid_blocks(W, H)) + T - 1) / T;
}
// A 256-thread level never needs a third slot: it has at most (kIcpMaxBlocks - 1) * kIcpThreads pixels (icp_threads_for), and once its grid is
// capped the chunk is that over kIcpGeoCap256 workgroups, rounded up to 64 -- 384 pixels.  So the 256-thread dispatch has two forms.
static_assert(((((kIcpMaxBlocks - 1) * kIcpThreads + kIcpGeoCap256 - 1) / kIcpGeoCap256 + 63) / 64) * 64 <= 2 * 256,
              "a 256-thread level would need k_icp_iter<256, 3>");

// the form launch_icp_iteration gives a level of W x H pixels (what it launches, and what mf_k_icp_launch_form reports)
IcpForm icp_launch_form(int W, int H) {
    IcpForm f;
    const int P = W * H;
    f.threads = icp_threads_for(P);
    f.slots = icp_pixel_slots(W, H);
    f.blocks = icp_geo_grid_blocks(W, H);
    f.chunk = icp_chunk(P, f.blocks);
    f.live = (P + f.chunk - 1) / f.chunk;   // workgroups whose chunk starts inside the image
    return f;
}

void launch_icp_iteration(const IcpLaunch& l, hipStream_t s) {
    IcpKArgs a;
    a.vc = l.vmap_curr; a.nc = l.nmap_curr; a.vp = l.vmap_prev; a.np = l.nmap_prev;
    a.W = l.W; a.H = l.H; a.k = l.k; icp_gates(l.distThres, l.angleThres, a.dist2Max, a.sine2Min);
    a.partials_in = l.partials_in; a.nb_in = l.nblocks_in; a.partials_out = l.partials_out;
    a.st_in = l.state_in; a.st_out = l.state_out; a.log_out = l.log_out; a.prof_out = l.prof_out; a.pose_in = l.pose_in;
    a.trace = l.trace; a.it = l.it;
    a.so3_in = l.so3_in;
    const IcpForm f = icp_launch_form(l.W, l.H);
    const dim3 grid(f.blocks);
    const int px = f.slots;
    if (f.threads == 256) {
        if (px <= 1) hipLaunchKernelGGL((k_icp_iter<256, 1>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_icp_iter<256, 2>), grid, dim3(256), 0, s, a);   // (never three: the static_assert above)
    } else {
        if (px <= 2) hipLaunchKernelGGL((k_icp_iter<kIcpThreads, 2>), grid, dim3(kIcpThreads), 0, s, a);
        else hipLaunchKernelGGL((k_icp_iter<kIcpThreads, kIcpPx>), grid, dim3(kIcpThreads), 0, s, a);
    }
}

// ------------------------------------------------------------------------------------------------
// begin / finalize
// ------------------------------------------------------------------------------------------------
// last reduce + solve of a tracking step, then Model::pose / lastPose / statistics (RGBDOdometry.cpp:476-496, Model.cpp:437-446)
// and the object-model jump rule.  Called by all 256 threads of a workgroup.
// one thread: the model's pose block and its pinned mirror from the final state (the fields a tracking step does not own keep their values)
// (the two blocks as restrict PARAMETERS: the compiler then carries the untouched fields from *pose to both stores in registers)
__device__ __forceinline__ void write_pose(PoseDev* __restrict__ pose, PoseDev* __restrict__ host_mirror, const GNState& st, const GnFinalize& f,
                                           bool photometric) {
    PoseDev p = *pose;
    pose_from_state(st, f.so3, f.jump_limit, photometric, p);
    *pose = p;
    if (host_mirror) *host_mirror = p;
}

// f.log: where the last reduced system goes (or nullptr).  s_st: the workgroup's LDS copy of the state.
__device__ __forceinline__ void icp_finalize_body(const float* __restrict__ partials_in, int nb_in, const GNState* st_in, const GnFinalize& f,
                                                  double* s_seg, double* s_sys, GNState* s_st, float* s_pose) {
    if (nb_in > 0) {
        gn_step_wg(st_in, partials_in, nb_in, s_seg, s_sys, s_st, s_pose);
        if (f.log && threadIdx.x >= 64 && threadIdx.x < 96) f.log[threadIdx.x - 64] = (float)s_sys[threadIdx.x - 64];
    } else {
        gn_stage(s_st, st_in);
    }
    __syncthreads();
    gn_trace_write(f.trace, f.n_it, nb_in > 0, s_sys, s_st, (int)threadIdx.x - 128);   // the last system and the state it led to
    if (threadIdx.x == 0) write_pose(f.pose, f.host_mirror, *s_st, f, false);
}

// (GnFinalize's fields arrive as restrict parameters of their own: inside a by-value struct they are not, and the kernel took 130 registers for 126)
__global__ __launch_bounds__(256) void k_icp_finalize(const float* __restrict__ partials_in, int nb_in, const GNState* __restrict__ st_in,
                                                       PoseDev* __restrict__ pose, PoseDev* __restrict__ host_mirror, float* __restrict__ log_out,
                                                       float jump_limit, const So3Result* __restrict__ so3, double* __restrict__ trace, int n_it) {
    const GnFinalize f{pose, host_mirror, log_out, jump_limit, so3, trace, n_it};
    __shared__ double s_seg[32 * 32];
    __shared__ double s_sys[32];
    __shared__ GNState s_st;
    __shared__ float s_pose[24];
    icp_finalize_body(partials_in, nb_in, st_in, f, s_seg, s_sys, &s_st, s_pose);
}

void launch_icp_finalize(const GnLast& last, const GnFinalize& f, hipStream_t s) {
    hipLaunchKernelGGL(k_icp_finalize, dim3(1), dim3(256), 0, s, last.partials, last.nblocks, last.state, f.pose, f.host_mirror, f.log, f.jump_limit, f.so3,
                       f.trace, f.n_it);
}

// ------------------------------------------------------------------------------------------------
// Batched Gauss-Newton loop: iteration k of ALL tracked models per launch (see mf_internal.h).
// ------------------------------------------------------------------------------------------------
struct IcpSolveArgs { TrackBatch b; int it; int nb_in; const So3Result* so3; };

// One model's step between two pixel passes of the batched loop, by all threads of a workgroup: it == 0 seeds the state, it > 0 finishes iteration
// it - 1 (the functions k_icp_iter's prologue calls, on the same data in the same order: the same bits).  publish: this workgroup also leaves state,
// log and trace in the model's block.  s_st is ready for every thread on return.
__device__ __forceinline__ void batch_step(const TrackModelDev& md, int it, int nb_in, const So3Result* so3, bool publish, double* s_seg, double* s_sys,
                                           GNState* s_st, float* s_pose) {
    if (it == 0) {
        if (threadIdx.x == 0) gn_seed(*md.pose, so3, *s_st);
    } else {
        const int prev = (it - 1) & 1;
        gn_step_wg(md.st + prev, md.partials[prev], nb_in, s_seg, s_sys, s_st, s_pose);
    }
    __syncthreads();
    // (it == 0: no system was reduced -- s_sys holds nothing, and have_sys = false keeps gn_publish from reading it)
    if (publish) gn_publish(md.st + (it & 1), (md.log && it > 0) ? md.log + 32 * (it - 1) : nullptr, md.trace, it, it > 0, s_sys, s_st);
}

__global__ __launch_bounds__(256) void k_icp_batch_solve(const IcpSolveArgs a) {
    __shared__ double s_seg[32 * 32];
    __shared__ double s_sys[32];
    __shared__ GNState s_st;
    __shared__ float s_pose[24];
    batch_step(*a.b.m[blockIdx.x], a.it, a.nb_in, a.so3, true, s_seg, s_sys, &s_st, s_pose);
}

struct IcpPxArgs {
    TrackBatch b;
    const float* vc; const float* nc;
    int W, H; Intr k;
    float dist2Max, sine2Min;
    int level, parity, chunk;
    const float2* row_z;      // [H] {min z, max z} of the valid vertices of every row of vc (launch_row_zrange); nullptr: no slab culling
    // fused != 0 ("batchSolveInPixelPass"): the launch finishes the previous iteration itself -- every workgroup of a model reduces that model's partial
    // sums and solves, identically, as k_icp_iter's prologue does for a single model -- instead of reading the state k_icp_batch_solve wrote
    int fused, it, nb_in; const So3Result* so3;
};

// {min z, max z} over the valid vertices of every row of the three levels' vertex maps (planar [3][H][W]: z is plane 2)
struct RowZArgs { const float* vm[3]; int W, H; float2* out; };
__global__ __launch_bounds__(64) void k_row_zrange(const RowZArgs a) {
    int row = blockIdx.x, level = 0, W = a.W, H = a.H, base = 0;
    while (level < 2 && row >= H) { row -= H; base += H; W >>= 1; H >>= 1; ++level; }
    const float* __restrict__ z = a.vm[level] + 2 * (size_t)W * H + (size_t)row * W;
    float lo = INFINITY, hi = -INFINITY;
    for (int x = threadIdx.x; x < W; x += 64) {
        const float v = z[x];
        if (v == v) { lo = fminf(lo, v); hi = fmaxf(hi, v); }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { lo = fminf(lo, __shfl_xor(lo, off, 64)); hi = fmaxf(hi, __shfl_xor(hi, off, 64)); }
    if (threadIdx.x == 0) a.out[base + row] = make_float2(lo, hi);
}
void launch_row_zrange(const float* const vmap[3], int W, int H, float2* out, hipStream_t s) {
    RowZArgs a{{vmap[0], vmap[1], vmap[2]}, W, H, out};
    hipLaunchKernelGGL(k_row_zrange, dim3(H + (H >> 1) + (H >> 2)), dim3(64), 0, s, a);
}
constexpr int kBatchThreads = 256;
constexpr int kBatchPx = 3;   // pixels per thread and round: all their gathers are in flight together

__global__ __launch_bounds__(kBatchThreads) void k_icp_batch_pixels(const IcpPxArgs a) {
    __shared__ float s_red[29 * (kBatchThreads / 2)];
    __shared__ double s_seg[32 * 32];
    __shared__ double s_sys[32];
    __shared__ GNState s_st;
    __shared__ float s_pose[24];
    const TrackModelDev* __restrict__ md = a.b.m[blockIdx.y];
    const float* __restrict__ vp = md->vm[a.level];
    const float* __restrict__ np = md->nm[a.level];
    const int tid = threadIdx.x;
    if (a.fused) {
        // k_icp_batch_solve's work as this launch's prologue, in every workgroup of the model; workgroup 0 of the model publishes state, log and trace
        // for the next launch and the finalize step.  One launch per iteration instead of two: a dependent launch is 3.4 us before it does anything
        batch_step(*md, a.it, a.nb_in, a.so3, blockIdx.x == 0, s_seg, s_sys, &s_st, s_pose);
    } else {
        gn_stage(&s_st, md->st + a.parity);
        __syncthreads();
    }
    const GNState* st = &s_st;
    float Rc[9], Rpi[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Rc[k] = st->Rcurr[k]; Rpi[k] = st->Rprev_inv[k]; }
    const float3 tc = f3(st->tcurr[0], st->tcurr[1], st->tcurr[2]);
    const float3 tp = f3(st->tprev[0], st->tprev[1], st->tprev[2]);
    const int P = a.W * a.H;
    const int beg = blockIdx.x * a.chunk, end = min(P, beg + a.chunk);
    // Slab culling (exact).  A frame pixel contributes only if it projects onto a pixel of the model's maps that holds a normal (reduce.cu:316-352:
    // everything else is a NaN reject), and an OBJECT's maps hold normals on the object alone -- ~1 % of the image (Q3).  The workgroup's pixels
    // are rows r0 .. r1 of the frame's vertex map; every valid vertex of those rows lies on the ray of its pixel at a depth inside the rows' range
    // [zmin, zmax] (row_z), i.e. inside the frustum section spanned by the four corner rays of the row band between those depths -- a convex
    // set, the hull of its eight corners.  The iteration's relative pose maps it to the hull of the transformed corners; if all of them lie in front
    // of the model camera, the projection of a convex set is inside the convex hull of the projected corners, hence inside their bounding box.
    // If that box (grown by 2 px against the rounding of the per-pixel arithmetic) misses the model's rectangle of normals (TrackModelDev::rect,
    // grown likewise), no pixel of the workgroup can find a correspondence: its partial sums are zero, written without touching a map.
    __shared__ int s_skip;
    if (a.row_z && beg < end && !md->allow_fill) {     // (the background's prediction covers the image: nothing to cull)
        if (tid < 64) {
            const int r0 = beg / a.W, r1 = (end - 1) / a.W;
            float zlo = INFINITY, zhi = -INFINITY;
            for (int r = r0 + tid; r <= r1; r += 64) { const float2 z = a.row_z[r]; zlo = fminf(zlo, z.x); zhi = fmaxf(zhi, z.y); }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { zlo = fminf(zlo, __shfl_xor(zlo, off, 64)); zhi = fmaxf(zhi, __shfl_xor(zhi, off, 64)); }
            // lanes 0..7: corner (x side, row side, depth end) of the slab
            const float cxs = (tid & 1) ? (float)(a.W - 1) : 0.f, cys = (tid & 2) ? (float)r1 : (float)r0, cz = (tid & 4) ? zhi : zlo;
            const float3 p = f3(cz * (cxs - a.k.cx) / a.k.fx, cz * (cys - a.k.cy) / a.k.fy, cz);           // createVMap, cudafuncs.cu:118-123
            const float3 g = icp_mul33(Rc, p);
            const float3 q = icp_mul33(Rpi, f3(g.x + tc.x - tp.x, g.y + tc.y - tp.y, g.z + tc.z - tp.z));
            const bool front = q.z > 1e-3f;
            float u = front ? q.x * a.k.fx / q.z + a.k.cx : 0.f, v = front ? q.y * a.k.fy / q.z + a.k.cy : 0.f;
            float ulo = tid < 8 ? u : INFINITY, uhi = tid < 8 ? u : -INFINITY, vlo = tid < 8 ? v : INFINITY, vhi = tid < 8 ? v : -INFINITY;
            int all_front = (tid >= 8 || front) ? 1 : 0;
#pragma unroll
            for (int off = 4; off > 0; off >>= 1) {
                ulo = fminf(ulo, __shfl_xor(ulo, off, 64)); uhi = fmaxf(uhi, __shfl_xor(uhi, off, 64));
                vlo = fminf(vlo, __shfl_xor(vlo, off, 64)); vhi = fmaxf(vhi, __shfl_xor(vhi, off, 64));
                all_front &= __shfl_xor(all_front, off, 64);
            }
            if (tid == 0) {
                // (level-0 rectangle: a coarser level's normals lie inside it shifted right by the level -- k_model_pyramid)
                const int rc0 = md->rect[0], rc1 = md->rect[1], rc2 = md->rect[2], rc3 = md->rect[3];
                bool skip = !(zlo <= zhi);                                        // no valid vertex in these rows at all
                if (!skip && all_front && ulo == ulo && uhi == uhi && vlo == vlo && vhi == vhi) {
                    const bool empty = rc0 > rc2 || rc1 > rc3;                   // the model's maps hold no normal
                    skip = empty || uhi + 2.5f < (float)(rc0 >> a.level) || ulo - 2.5f > (float)(rc2 >> a.level) || vhi + 2.5f < (float)(rc1 >> a.level) ||
                           vlo - 2.5f > (float)(rc3 >> a.level);
                }
                s_skip = skip ? 1 : 0;
            }
        }
        __syncthreads();
        if (s_skip) {
            if (tid < kIcpSlots) md->partials[a.parity][blockIdx.x * kIcpSlots + tid] = 0.f;
            return;
        }
    }
    float acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.f;
    static_assert(kBatchPx == 3, "kAllSlots names every slot");
    const bool kAllSlots[kBatchPx] = {true, true, true};   // (no wavefront of a round idles: the chunk is a multiple of the round)
    for (int base = beg; base < end; base += kBatchPx * kBatchThreads) {
        bool act[kBatchPx];
        IcpPx px[kBatchPx];
#pragma unroll
        for (int q = 0; q < kBatchPx; ++q) {
            const int i0 = base + q * kBatchThreads + tid;
            act[q] = i0 < end;
            const int i = min(i0, P - 1);      // masked slots re-read a valid pixel: no divergent control flow (see k_icp_iter)
            px[q] = IcpPx{a.vc[i], a.vc[P + i], a.vc[2 * P + i], a.nc[i], a.nc[P + i], a.nc[2 * P + i]};
        }
        icp_slots<kBatchPx>(px, act, kAllSlots, vp, np, P, Rc, tc, Rpi, tp, a, acc);
    }
    block_sum29_lds<kBatchThreads>(acc, s_red, md->partials[a.parity] + blockIdx.x * kIcpSlots);
}

struct IcpFinArgs { TrackBatch b; int n_it; int nb_in; const So3Result* so3; };
__global__ __launch_bounds__(256) void k_icp_batch_finalize(const IcpFinArgs a) {
    __shared__ double s_seg[32 * 32];
    __shared__ double s_sys[32];
    __shared__ GNState s_st;
    __shared__ float s_pose[24];
    const TrackModelDev* __restrict__ md = a.b.m[blockIdx.x];
    const int last = (a.n_it - 1) & 1;
    const GnFinalize f{md->pose, md->pose_host, (md->log && a.n_it > 0) ? md->log + 32 * (a.n_it - 1) : nullptr, md->jump_limit, a.so3, md->trace, a.n_it};
    icp_finalize_body(a.n_it > 0 ? md->partials[last] : nullptr, a.n_it > 0 ? a.nb_in : 0, md->st + (a.n_it > 0 ? last : 0), f, s_seg, s_sys, &s_st, s_pose);
    if (threadIdx.x < 4) md->rect[threadIdx.x] = (threadIdx.x & 2) ? (int)0x80000000 : 0x7FFFFFFF;   // armed for the next frame's model pyramid
}

// Workgroups per model of the pixel pass: enough of them over all models to fill the GPU a few times over (there is no
// per-workgroup prologue to amortise, only one 32-value halving tree per wavefront), never less than one round of pixels.
int icp_batch_max_blocks(int W, int H) { return (W * H + kBatchPx * kBatchThreads - 1) / (kBatchPx * kBatchThreads); }
static int icp_batch_chunk(int P, int n_models) {
    const int round = kBatchPx * kBatchThreads;
    int per_model = (768 + n_models - 1) / n_models;                  // ~3 workgroups per CU in total
    int chunk = (P + per_model - 1) / per_model;
    chunk = ((chunk + round - 1) / round) * round;
    return chunk < round ? round : chunk;
}
int icp_batch_blocks(int W, int H, int n_models) {
    const int P = W * H, chunk = icp_batch_chunk(P, n_models);
    return (P + chunk - 1) / chunk;
}
void launch_icp_batch_solve(const TrackBatch& b, int it, int nb_in, const So3Result* so3, hipStream_t s) {
    IcpSolveArgs a{b, it, nb_in, so3};
    hipLaunchKernelGGL(k_icp_batch_solve, dim3(b.n), dim3(256), 0, s, a);
}
void launch_icp_batch_pixels(const TrackBatch& b, int it, const IcpBatchLevel& l, bool fused, int nb_in, const So3Result* so3, hipStream_t s) {
    IcpPxArgs a;
    a.row_z = l.row_z;
    a.fused = fused ? 1 : 0; a.it = it; a.nb_in = nb_in; a.so3 = so3;
    a.b = b; a.vc = l.vmap_curr; a.nc = l.nmap_curr; a.W = l.W; a.H = l.H; a.k = l.k; icp_gates(l.distThres, l.angleThres, a.dist2Max, a.sine2Min);
    a.level = l.level; a.parity = it & 1; a.chunk = icp_batch_chunk(l.W * l.H, b.n);
    hipLaunchKernelGGL(k_icp_batch_pixels, dim3(icp_batch_blocks(l.W, l.H, b.n), b.n), dim3(kBatchThreads), 0, s, a);
}
void launch_icp_batch_finalize(const TrackBatch& b, int n_it, int nb_in, const So3Result* so3, hipStream_t s) {
    IcpFinArgs a{b, n_it, nb_in, so3};
    hipLaunchKernelGGL(k_icp_batch_finalize, dim3(b.n), dim3(256), 0, s, a);
}

// stand-alone Gauss-Newton update for the parity tests (mf_k_gn_solve): the production one-thread path (unpack -> LDL^T -> exp ->
// pose composition) and the wave-parallel Gauss-Jordan of the RGB-D kernels on the same system
struct GnSolveOut { double x_serial[6], x_wave[6], resultRt[16]; float Rcurr[9], tcurr[3], trR[9], trt[3], lastICPError, lastICPCount; };
__global__ __launch_bounds__(128) void k_gn_solve_test(const double* __restrict__ sys29, const double* __restrict__ resultRt,
                                                      const float* __restrict__ Rprev, const float* __restrict__ tprev, GnSolveOut* out) {
    __shared__ double s_sys[32];
    __shared__ GNState s_st;
    __shared__ float s_pose[24];
    if (threadIdx.x < 32) s_sys[threadIdx.x] = threadIdx.x < 29 ? sys29[threadIdx.x] : 0.0;
    if (threadIdx.x == 0) {   // a seed from the pose [Rprev | tprev], but for the given resultRt
        PoseDev p;
        for (int k = 0; k < 9; ++k) p.R[k] = Rprev[k];
        for (int k = 0; k < 3; ++k) p.t[k] = tprev[k];
        gn_seed(p, nullptr, s_st);
        for (int k = 0; k < 16; ++k) s_st.resultRt[k] = resultRt[k];
    }
    __syncthreads();
    double xw[6];
    solve6_wave(s_sys, xw);
    // what k_icp_iter / k_icp_batch_solve / k_icp_finalize call: twelve lanes, state in LDS (the serial form -- gn_solve_update_serial --
    // stays as the executable specification: tests/test_devmath_host.py compiles it for the host)
    gn_finish_wg(s_sys, &s_st, s_pose);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double A[6][6], b[6], x[6];
    int shift = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 7; ++j) {
            const double value = s_sys[shift++];
            if (j == 6) b[i] = value;
            else { A[i][j] = value; A[j][i] = value; }
        }
    ldlt6_solve(A, b, x);
    const GNState& st = s_st;
    for (int k = 0; k < 6; ++k) { out->x_serial[k] = x[k]; out->x_wave[k] = xw[k]; }
    for (int k = 0; k < 16; ++k) out->resultRt[k] = st.resultRt[k];
    for (int k = 0; k < 9; ++k) { out->Rcurr[k] = st.Rcurr[k]; out->trR[k] = st.trR[k]; }
    for (int k = 0; k < 3; ++k) { out->tcurr[k] = st.tcurr[k]; out->trt[k] = st.trt[k]; }
    out->lastICPError = st.lastICPError; out->lastICPCount = st.lastICPCount;
}
int gn_solve_standalone(const double* sys29, const double* resultRt16, const float* Rprev9, const float* tprev3, double* x_serial, double* x_wave,
                        double* resultRt_out, float* Rcurr9, float* tcurr3, float* stats2, hipStream_t s) {
    char* buf = nullptr;
    const size_t in_bytes = 29 * 8 + 16 * 8 + 12 * 4;
    if (hipMalloc((void**)&buf, in_bytes + sizeof(GnSolveOut)) != hipSuccess) return -1;
    double* d_sys = reinterpret_cast<double*>(buf);
    double* d_rt = d_sys + 29;
    float* d_R = reinterpret_cast<float*>(d_rt + 16);
    GnSolveOut* d_out = reinterpret_cast<GnSolveOut*>(buf + in_bytes);
    GnSolveOut h;
    bool ok = hipMemcpyAsync(d_sys, sys29, 29 * 8, hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemcpyAsync(d_rt, resultRt16, 16 * 8, hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemcpyAsync(d_R, Rprev9, 36, hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemcpyAsync(d_R + 9, tprev3, 12, hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_gn_solve_test, dim3(1), dim3(128), 0, s, d_sys, d_rt, d_R, d_R + 9, d_out);   // two wavefronts: gn_finish_wg's statistics run in the second
        ok = hipMemcpyAsync(&h, d_out, sizeof(h), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    (void)hipFree(buf);
    if (!ok) return -2;
    memcpy(x_serial, h.x_serial, 48); memcpy(x_wave, h.x_wave, 48); memcpy(resultRt_out, h.resultRt, 128);
    memcpy(Rcurr9, h.Rcurr, 36); memcpy(tcurr3, h.tcurr, 12);
    stats2[0] = h.lastICPError; stats2[1] = h.lastICPCount;
    return 0;
}

// stand-alone icpStep for the parity tests: reduce partials to 32 floats
__global__ __launch_bounds__(256) void k_icp_reduce_only(const float* __restrict__ partials, int nb, float* __restrict__ out32) {
    __shared__ double s_seg[32 * 32];
    __shared__ double s_sys[32];
    reduce_partials(partials, nb, s_seg, s_sys);
    if (threadIdx.x < 32) out32[threadIdx.x] = (float)s_sys[threadIdx.x];
}

__global__ void k_state_from_args(GNState* st, const float* Rc, const float* tc, const float* Rpi, const float* tp) {
    if (threadIdx.x != 0) return;
    GNState s;   // a seed from the pose [Rc | tc], but for the given previous pose's inverse rotation and translation
    PoseDev p;
    for (int k = 0; k < 9; ++k) p.R[k] = Rc[k];
    for (int k = 0; k < 3; ++k) p.t[k] = tc[k];
    gn_seed(p, nullptr, s);
    for (int k = 0; k < 9; ++k) s.Rprev_inv[k] = Rpi[k];
    for (int k = 0; k < 3; ++k) s.tprev[k] = tp[k];
    *st = s;
}

void launch_icp_step_standalone(const float* Rcurr, const float* tcurr, const float* vc, const float* nc, const float* Rpi,
                                const float* tprev, Intr k, const float* vp, const float* np, float distThres,
                                float angleThres, int W, int H, float* partials, GNState* st, float* out32, hipStream_t s) {
    // partials: scratch of icp_geo_grid_blocks(W,H) * 32 floats; st: two GNState
    hipLaunchKernelGGL(k_state_from_args, dim3(1), dim3(64), 0, s, st, Rcurr, tcurr, Rpi, tprev);
    IcpLaunch l;
    l.vmap_curr = vc; l.nmap_curr = nc; l.vmap_prev = vp; l.nmap_prev = np; l.W = W; l.H = H; l.k = k;
    l.distThres = distThres; l.angleThres = angleThres; l.partials_in = nullptr; l.nblocks_in = 0;
    l.partials_out = partials; l.state_in = st; l.state_out = st + 1; l.log_out = nullptr; l.prof_out = nullptr;
    launch_icp_iteration(l, s);
    hipLaunchKernelGGL(k_icp_reduce_only, dim3(1), dim3(256), 0, s, partials, icp_geo_grid_blocks(W, H), out32);
}

// The same stand-alone icpStep through the OTHER kernels that inline icp_project / icp_accumulate (tests/test_gpu_gn_gates.py), each launched by the
// production launch function and reduced by k_icp_reduce_only into the same 32 floats:
//   form 1  k_icp_batch_pixels for a one-model TrackBatch, unfused, no row_z (every workgroup walks its pixels)
//   form 2  form 1 with row_z from launch_row_zrange, allow_fill = 0 and the given level-0 rectangle of model normals: the slab culling
//   form 3  k_rgbd_iter with icpOn = 1 on a blank photometric level (zero images: no photometric correspondence), followed by its k_rgb_step
// dpose: device Rcurr[9] tcurr[3] Rprev_inv[9] tprev[3].  Allocates and frees its own scratch; synchronous.  Returns 0, -1 (no memory), -2 (HIP error).
int icp_step_form_standalone(int form, const float* dpose, const float* vc, const float* nc, Intr k, const float* vp, const float* np, float distThres,
                             float angleThres, int W, int H, const int* rect4, float* out32, hipStream_t s) {
    const size_t P = (size_t)W * H;
    const int nb = form == 3 ? icp_grid_blocks(W, H) : icp_batch_blocks(W, H, 1);
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t b_part = up16((size_t)nb * kIcpSlots * sizeof(float)), b_st = up16(2 * sizeof(GNState));
    const size_t n_rowz = (size_t)H + (H >> 1) + (H >> 2);
    const size_t b_rest = form == 3 ? b_part + up16((size_t)nb * sizeof(int2)) + up16(P * sizeof(RgbCorr)) + up16(P * sizeof(float))
                                    : up16(sizeof(TrackModelDev)) + up16(4 * sizeof(int)) + up16(n_rowz * sizeof(float2));
    char* base = nullptr;
    if (hipMalloc((void**)&base, b_part + b_st + b_rest) != hipSuccess) return -1;
    float* partials = reinterpret_cast<float*>(base);
    GNState* st = reinterpret_cast<GNState*>(base + b_part);
    char* rest = base + b_part + b_st;
    hipLaunchKernelGGL(k_state_from_args, dim3(1), dim3(64), 0, s, st, dpose, dpose + 9, dpose + 12, dpose + 21);
    bool ok = true;
    if (form == 3) {
        float* rgb_partials = reinterpret_cast<float*>(rest);
        int2* cnt = reinterpret_cast<int2*>(rest + b_part);
        RgbCorr* corres = reinterpret_cast<RgbCorr*>(rest + b_part + up16((size_t)nb * sizeof(int2)));
        char* zeros = reinterpret_cast<char*>(corres) + up16(P * sizeof(RgbCorr));   // every image of the blank level: P zero floats / shorts / bytes
        ok = hipMemsetAsync(zeros, 0, P * sizeof(float), s) == hipSuccess;
        RgbdLaunch r;
        IcpLaunch& l = r.icp;
        l.vmap_curr = vc; l.nmap_curr = nc; l.vmap_prev = vp; l.nmap_prev = np; l.W = W; l.H = H; l.k = k;
        l.distThres = distThres; l.angleThres = angleThres; l.partials_in = nullptr; l.nblocks_in = 0;
        l.partials_out = partials; l.state_in = st; l.state_out = st + 1; l.log_out = nullptr;
        RgbLevel& L = r.L;
        L.dIdx = reinterpret_cast<const int16_t*>(zeros); L.dIdy = L.dIdx;
        L.lastDepth = reinterpret_cast<const float*>(zeros); L.nextDepth = L.lastDepth;
        L.lastImage = reinterpret_cast<const uint8_t*>(zeros); L.nextImage = L.lastImage;
        L.W = W; L.H = H; L.minScale = 0.f; L.maxDepthDelta = 0.07f; L.gate = nullptr;
        r.corres = corres; r.rgb_partials_in = nullptr; r.rgb_partials_out = rgb_partials; r.cnt_in = nullptr; r.cnt_out = cnt;
        r.icpWeight = 10.f; r.icpOn = 1; r.rgbOnly = 0; r.sobelScale = 0.125f; r.level = 0; r.prev_level = 0; r.so3_in = nullptr;
        if (ok) launch_rgbd_iteration(r, s);
    } else {
        TrackModelDev* d_md = reinterpret_cast<TrackModelDev*>(rest);
        int* d_rect = reinterpret_cast<int*>(rest + up16(sizeof(TrackModelDev)));
        float2* d_rowz = reinterpret_cast<float2*>(rest + up16(sizeof(TrackModelDev)) + up16(4 * sizeof(int)));
        TrackModelDev md;
        memset(&md, 0, sizeof(md));
        md.vm[0] = const_cast<float*>(vp); md.nm[0] = const_cast<float*>(np);
        md.partials[0] = partials; md.partials[1] = partials; md.st = st; md.allow_fill = 0; md.rect = d_rect;
        const int full[4] = {0, 0, W - 1, H - 1};
        ok = hipMemcpyAsync(d_md, &md, sizeof(md), hipMemcpyHostToDevice, s) == hipSuccess &&
             hipMemcpyAsync(d_rect, rect4 ? rect4 : full, sizeof(full), hipMemcpyHostToDevice, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;   // md and full are stack buffers
        if (ok && form == 2) {
            // (only level 0's ranges are read; the coarser levels' rows are computed from planes inside the same map: [2 P / 4, 3 P / 4) and [2 P / 16, 3 P / 16))
            const float* const vm3[3] = {vc, vc, vc};
            launch_row_zrange(vm3, W, H, d_rowz, s);
        }
        TrackBatch b;
        memset(&b, 0, sizeof(b));
        b.m[0] = d_md; b.n = 1;
        const IcpBatchLevel lv{0, vc, nc, W, H, k, distThres, angleThres, form == 2 ? d_rowz : nullptr};
        if (ok) launch_icp_batch_pixels(b, 0, lv, false, 0, nullptr, s);
    }
    if (ok) hipLaunchKernelGGL(k_icp_reduce_only, dim3(1), dim3(256), 0, s, partials, nb, out32);
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    (void)hipFree(base);
    return ok && hipGetLastError() == hipSuccess ? 0 : -2;
}

// ------------------------------------------------------------------------------------------------
// RGB-D Gauss-Newton loop (icpWeight < 100 or rgbOnly): two launches per iteration.
//   A  k_rgbd_iter : [finish the previous iteration: reduce ICP + RGB partials, combine, solve, pose] ->
//                    ICP normal equations + photometric correspondences (RgbCorr per pixel, count / sum diff^2)
//   B  k_rgb_step  : [sigma = reduced count] -> photometric normal equations from the correspondences
// B exists because the photometric weight 1 / (count + |diff|) needs the GLOBAL correspondence count of the same
// iteration (RGBDOdometry.cpp:389-401,436); a launch boundary is the only grid-wide ordering point used here.
// The ICP-only loop keeps its own tuned kernel (k_icp_iter).
// ------------------------------------------------------------------------------------------------
struct RgbdKArgs {
    IcpKArgs icp;                 // maps, intrinsics, thresholds, ICP partials in/out, state in/out, pose_in
    RgbLevel L;                   // photometric inputs of THIS launch's level
    RgbCorr* corres;              // [W*H] out
    const float* rgb_partials_in; // [nb_in][32]  (B of the previous iteration)
    const int2* cnt_in;           // [nb_in]      (A of the previous iteration): {count, sum diff^2}
    int2* cnt_out;                // [gridDim.x]
    float icpWeight; int icpOn; int rgbOnly;
    int level, prev_level;
    const So3Result* so3_in;      // first launch: rotation seed of resultRt (nullptr: identity)
};

__device__ __forceinline__ float rgb_tmp_error(int count, int sigma) {  // RGBDOdometry.cpp:389
    return (float)(sqrt((double)sigma) / (double)count);
}

// Finishes the iteration whose partial sums are given; every workgroup calls it with all threads and gets the same
// answer.  Returns true in the one thread (0) that holds `out`.
__device__ __forceinline__ bool finish_rgbd_iteration(const float* icp_partials, const float* rgb_partials, const int2* cnt, int nb,
                                                      float icpWeight, int icpOn, int rgbOnly, int prev_level, const GNState& in,
                                                      GNState& out, double* s_seg, double* s_seg2, double* s_sys, double* s_sys2,
                                                      int* s_cnt, float* log_out) {
    if (blockDim.x >= 512) {
        reduce_partials_pair(icp_partials, rgb_partials, cnt, nb, s_seg, s_seg2, s_sys, s_sys2, s_cnt);
    } else {
        reduce_partials(icp_partials, nb, s_seg, s_sys);
        reduce_partials(rgb_partials, nb, s_seg, s_sys2);
        reduce_counts(cnt, nb, s_cnt);
    }
    if (threadIdx.x >= 64) return false;
    double x[6];
    const double w = (double)icpWeight;
    solve6_wave_rgbd(s_sys, s_sys2, icpOn ? w * w : 0.0, icpOn ? w : 0.0, x);
    if (threadIdx.x != 0) return false;
    if (in.levelDone == prev_level) { out = in; return true; }             // that level's loop was already left
    const int count = s_cnt[0], sigma = s_cnt[1];
    const float tmpError = rgb_tmp_error(count, sigma);
    if (rgbOnly && tmpError > in.lastRGBError) {                            // RGBDOdometry.cpp:392-394: break
        out = in;
        out.levelDone = prev_level;
        return true;
    }
    gn_update_from_x(x, (float)s_sys[27], (float)s_sys[28], in, out);
    if (!icpOn) { out.lastICPError = in.lastICPError; out.lastICPCount = in.lastICPCount; }
    out.lastRGBError = tmpError;
    out.lastRGBCount = (float)count;
    if (log_out)
        for (int k = 0; k < 32; ++k) log_out[k] = (float)s_sys2[k];
    return true;
}

__global__ __launch_bounds__(kIcpThreads) void k_rgbd_iter(const RgbdKArgs a) {
    __shared__ double s_seg[32 * 32];
    __shared__ double s_seg2[32 * 32];
    __shared__ double s_sys[32];
    __shared__ double s_sys2[32];
    __shared__ float s_pose[24];   // Rcurr[9] tcurr[3] Rprev_inv[9] tprev[3]
    __shared__ float s_krk[12];    // K R K^-1 [9], K t [3] of this iteration
    __shared__ float s_part[(kIcpThreads / 64) * kIcpSlots];
    __shared__ int s_cnt[2];
    __shared__ int s_icnt[(kIcpThreads / 64) * 2];
    __shared__ int s_skip;
    __shared__ GNState s_st;

    const int tid = threadIdx.x;
    const IcpKArgs& ia = a.icp;
    if (ia.pose_in == nullptr) gn_stage(&s_st, ia.st_in);
    else if (tid == 0) gn_seed(*ia.pose_in, a.so3_in, s_st);
    __syncthreads();
    const int P = ia.W * ia.H;
    const int chunk = icp_chunk(P, gridDim.x);
    const int beg = blockIdx.x * chunk, end = min(P, beg + chunk);

    // prologue: finish the previous iteration, then derive what this iteration needs
    GNState st;
    bool mine;
    if (ia.nb_in > 0) {
        mine = finish_rgbd_iteration(ia.partials_in, a.rgb_partials_in, a.cnt_in, ia.nb_in, a.icpWeight, a.icpOn, a.rgbOnly, a.prev_level,
                                     s_st, st, s_seg, s_seg2, s_sys, s_sys2, s_cnt, (blockIdx.x == 0) ? ia.log_out : nullptr);
    } else {
        mine = tid == 0;
        if (mine) st = s_st;
    }
    if (mine) {
        if (a.level != a.prev_level) st.lastRGBError = 3.4028234664e38f;   // RGBDOdometry.cpp:359
#pragma unroll
        for (int k = 0; k < 9; ++k) { s_pose[k] = st.Rcurr[k]; s_pose[12 + k] = st.Rprev_inv[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_pose[9 + k] = st.tcurr[k]; s_pose[21 + k] = st.tprev[k]; }
        float krk[9], kt[3];
        krk_from_result(st.resultRt, ia.k, krk, kt);
        for (int k = 0; k < 9; ++k) s_krk[k] = krk[k];
        for (int k = 0; k < 3; ++k) s_krk[9 + k] = kt[k];
        s_skip = st.levelDone == a.level;
        if (blockIdx.x == 0) *ia.st_out = st;
    }
    __syncthreads();
    const bool skip = s_skip != 0;
    const int lane = tid & 63, wave = tid >> 6;

    // ---- ICP normal equations (as k_icp_iter, <= 2 px per thread)
    float acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.f;
    if (a.icpOn && !skip) {
        float Rc[9], Rpi[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { Rc[k] = s_pose[k]; Rpi[k] = s_pose[12 + k]; }
        const float3 tc = f3(s_pose[9], s_pose[10], s_pose[11]);
        const float3 tp = f3(s_pose[21], s_pose[22], s_pose[23]);
        for (int i = beg + tid; i < end; i += kIcpThreads) {
            const IcpCorr c = icp_project(ia.vc[i], ia.vc[P + i], ia.vc[2 * P + i], ia.nc[i], ia.nc[P + i], ia.nc[2 * P + i], Rc, tc, Rpi,
                                          tp, ia);
            const int j = c.j;
            const float3 pv = f3(ia.vp[j], ia.vp[P + j], ia.vp[2 * P + j]);
            const float3 pn = f3(ia.np[j], ia.np[P + j], ia.np[2 * P + j]);
            icp_accumulate(c, pv, pn, Rpi, tp, ia, acc);
        }
    }
    const float wsum = wave_sum32_halving(acc);
    if (lane < 32) s_part[wave * kIcpSlots + icp_component_of_lane(lane)] = wsum;

    // ---- photometric correspondences of this iteration
    unsigned cnt = 0, sig = 0;
    if (!skip) {
        float krk[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) krk[k] = s_krk[k];
        const float3 kt = f3(s_krk[9], s_krk[10], s_krk[11]);
        for (int i = beg + tid; i < end; i += kIcpThreads) {
            const int y = i / a.L.W, x = i - y * a.L.W;
            RgbCorr c;
            if (rgb_residual_px(a.L, krk, kt, x, y, c)) { cnt += 1u; sig += (unsigned)(int)(c.diff * c.diff); }
            a.corres[i] = c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cnt += (unsigned)__shfl_xor((int)cnt, o, 64); sig += (unsigned)__shfl_xor((int)sig, o, 64); }
    if (lane == 0) { s_icnt[wave * 2] = (int)cnt; s_icnt[wave * 2 + 1] = (int)sig; }
    __syncthreads();
    store_block_partial<kIcpThreads>(s_part, ia.partials_out);
    if (tid == 0) {
        unsigned c = 0, g = 0;
        for (int w = 0; w < kIcpThreads / 64; ++w) { c += (unsigned)s_icnt[w * 2]; g += (unsigned)s_icnt[w * 2 + 1]; }
        a.cnt_out[blockIdx.x] = make_int2((int)c, (int)g);
    }
}

struct RgbStepKArgs {
    RgbLevel L; Intr k; int level;
    const RgbCorr* corres; const int2* cnt_in; int nb;   // of the A launch of the same iteration
    const GNState* st;                                    // state written by that launch
    int rgbOnly; float sobelScale;
    float* partials_out;                                  // [gridDim.x][32]
};

__global__ __launch_bounds__(kIcpThreads) void k_rgb_step(const RgbStepKArgs a) {
    __shared__ float s_part[(kIcpThreads / 64) * kIcpSlots];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    reduce_counts(a.cnt_in, a.nb, s_cnt);
    const int count = s_cnt[0], sigma = s_cnt[1];
    const float tmpError = rgb_tmp_error(count, sigma);
    float sigmaVal = (tmpError == 0.f) ? 1.f : (float)count;   // RGBDOdometry.cpp:390
    if (a.rgbOnly) sigmaVal = -1.f;                             // :399-401
    const bool skip = a.st->levelDone == a.level;
    const int P = a.L.W * a.L.H;
    const int chunk = icp_chunk(P, gridDim.x);
    const int beg = blockIdx.x * chunk, end = min(P, beg + chunk);
    float acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.f;
    if (!skip) {
        for (int i = beg + tid; i < end; i += kIcpThreads) {
            const RgbCorr c = a.corres[i];
            if (c.u0 < 0) continue;
            const int y = i / a.L.W, x = i - y * a.L.W;
            rgb_step_px(a.L, c, x, y, sigmaVal, a.k, a.sobelScale, acc);
        }
    }
    const float wsum = wave_sum32_halving(acc);
    if (lane < 32) s_part[wave * kIcpSlots + icp_component_of_lane(lane)] = wsum;
    __syncthreads();
    store_block_partial<kIcpThreads>(s_part, a.partials_out);
}

struct RgbdFinKArgs {
    const float* icp_partials; const float* rgb_partials; const int2* cnt; int nb;   // of the last iteration (nb = 0: none ran)
    float icpWeight; int icpOn, rgbOnly, prev_level;
    const GNState* st_in;
    GnFinalize f;
};

__global__ __launch_bounds__(256) void k_rgbd_finalize(const RgbdFinKArgs a) {
    __shared__ double s_seg[32 * 32];
    __shared__ double s_sys[32];
    __shared__ double s_sys2[32];
    __shared__ int s_cnt[2];
    __shared__ GNState s_st;
    gn_stage(&s_st, a.st_in);
    __syncthreads();
    GNState st;
    bool mine;
    if (a.nb > 0) {
        mine = finish_rgbd_iteration(a.icp_partials, a.rgb_partials, a.cnt, a.nb, a.icpWeight, a.icpOn, a.rgbOnly, a.prev_level, s_st, st, s_seg, s_seg,
                                     s_sys, s_sys2, s_cnt, a.f.log);
    } else {
        mine = threadIdx.x == 0;
        if (mine) st = s_st;
    }
    if (mine) write_pose(a.f.pose, a.f.host_mirror, st, a.f, true);
}

void launch_rgbd_iteration(const RgbdLaunch& l, hipStream_t s) {
    RgbdKArgs a;
    const IcpLaunch& il = l.icp;
    a.icp.vc = il.vmap_curr; a.icp.nc = il.nmap_curr; a.icp.vp = il.vmap_prev; a.icp.np = il.nmap_prev;
    a.icp.W = il.W; a.icp.H = il.H; a.icp.k = il.k; icp_gates(il.distThres, il.angleThres, a.icp.dist2Max, a.icp.sine2Min);
    a.icp.partials_in = il.partials_in; a.icp.nb_in = il.nblocks_in; a.icp.partials_out = il.partials_out;
    a.icp.st_in = il.state_in; a.icp.st_out = il.state_out; a.icp.log_out = il.log_out; a.icp.prof_out = nullptr; a.icp.pose_in = il.pose_in; a.icp.so3_in = nullptr;
    a.L = l.L; a.corres = l.corres; a.rgb_partials_in = l.rgb_partials_in; a.cnt_in = l.cnt_in; a.cnt_out = l.cnt_out;
    a.icpWeight = l.icpWeight; a.icpOn = l.icpOn; a.rgbOnly = l.rgbOnly; a.level = l.level; a.prev_level = l.prev_level; a.so3_in = l.so3_in;
    const int nb = icp_grid_blocks(il.W, il.H);
    hipLaunchKernelGGL(k_rgbd_iter, dim3(nb), dim3(kIcpThreads), 0, s, a);
    RgbStepKArgs b;
    b.L = l.L; b.k = il.k; b.level = l.level; b.corres = l.corres; b.cnt_in = l.cnt_out; b.nb = nb; b.st = il.state_out;
    b.rgbOnly = l.rgbOnly; b.sobelScale = l.sobelScale; b.partials_out = l.rgb_partials_out;
    hipLaunchKernelGGL(k_rgb_step, dim3(nb), dim3(kIcpThreads), 0, s, b);
}

void launch_rgbd_finalize(const GnLast& last, float icpWeight, int icpOn, int rgbOnly, const GnFinalize& f, hipStream_t s) {
    const RgbdFinKArgs a{last.partials, last.rgb_partials, last.cnt, last.nblocks, icpWeight, icpOn, rgbOnly, last.level, last.state, f};
    hipLaunchKernelGGL(k_rgbd_finalize, dim3(1), dim3(256), 0, s, a);
}

}  // namespace mf
