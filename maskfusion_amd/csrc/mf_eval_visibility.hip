// mf_eval_visibility.hip -- run evaluation, which part of a cloud a sequence saw: every point of a cloud classified against every depth frame
// of a sequence (mf_cloud_visibility_dev; DESIGN.md "Cloud visibility").  No upstream twin: the reference scores nothing.  Third file of the
// evaluation family (mf_eval.hip: clouds against clouds, mf_eval_image.hip: images against images); it shares nothing with them but the
// compile flag below.
//
// Shape: one lane per point, the point and its four counters in registers, a loop over the call's frames, one row written at the end.  No
// atomics, no LDS, no second kernel.  Every lane of every workgroup walks the frames in the same order, so the frame the wavefronts are on
// (1.2 MB at 640 x 480) is what the L2 holds; the frame's 3 x 4 is indexed by the loop counter alone and comes through the scalar path
// (s_load_dwordx4 + s_load_dwordx8 per frame and wavefront).  A wavefront none of whose lanes is in front of the camera skips the two divisions, one
// none of whose lanes is in the frustum skips the depth load (s_cbranch_execz both times).  Everything that is stored is an integer count
// or a frame index: the result does not depend on the order of execution.  The fp32 arithmetic is rounded operation by operation in the
// order the header gives: this file is compiled without contraction (-ffp-contract=off, and the pragma for a build that forgets the flag).
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "../../include/maskfusion_amd.h"
#include "mf_internal.h"

namespace mf {

constexpr int kVisThreads = 256;

struct VisArgs {
    long long n;
    int stride, n_frames, H, W;
    float fx, fy, cx, cy, near_z, far_z, tol_abs, tol_rel;
    int frame_base, accumulate;
    int rows16;                               // d_counts is 16-byte aligned: a row is one 16-byte access
};

__global__ __launch_bounds__(kVisThreads) void k_cloud_visibility(const float* __restrict__ points, const float* __restrict__ depth,
                                                                  const float* __restrict__ cam, unsigned* __restrict__ counts,
                                                                  int* __restrict__ first, VisArgs a) {
    const long long i = (long long)blockIdx.x * kVisThreads + threadIdx.x;
    if (i >= a.n) return;
    const float* p = points + (size_t)i * (size_t)a.stride;
    const float x = p[0], y = p[1], z = p[2];
    const float fw = (float)a.W, fh = (float)a.H;          // at most 2^24: exact
    const size_t P = (size_t)a.W * (size_t)a.H;
    unsigned n_in = 0u, n_on = 0u, n_through = 0u, n_occluded = 0u;
    int f_on = -1;
    for (int f = 0; f < a.n_frames; ++f) {
        const float* M = cam + (size_t)f * 12;             // the same address in every lane: scalar loads
        const float zc = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
        if (!(zc > a.near_z && zc <= a.far_z)) continue;   // a NaN fails
        const float xc = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
        const float yc = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
        const float u = a.fx * (xc / zc) + a.cx;
        const float v = a.fy * (yc / zc) + a.cy;
        const float col = floorf(u + 0.5f), row = floorf(v + 0.5f);
        if (!(col >= 0.f && col < fw && row >= 0.f && row < fh)) continue;      // as floats: NaN and +-inf fail, and (int) is safe below
        ++n_in;
        const float d = depth[(size_t)f * P + (size_t)((int)row * a.W + (int)col)];
        if (!(d > 0.f && d <= 3.402823466e38f)) continue;  // a hole: not finite, or <= 0
        const float tol = a.tol_abs + a.tol_rel * d;
        const float dz = zc - d;
        if (fabsf(dz) <= tol) {
            ++n_on;
            if (f_on < 0) f_on = a.frame_base + f;
        } else if (dz < -tol) {
            ++n_through;
        } else if (dz > tol) {
            ++n_occluded;
        }
    }
    unsigned* out = counts + (size_t)i * 4;
    if (a.accumulate) {
        if (a.rows16) {
            const uint4 o = *(const uint4*)out;
            n_in += o.x; n_on += o.y; n_through += o.z; n_occluded += o.w;
        } else {
            n_in += out[0]; n_on += out[1]; n_through += out[2]; n_occluded += out[3];
        }
        const int f_old = first[i];
        if (f_old >= 0) f_on = f_old;
    }
    if (a.rows16) {
        *(uint4*)out = make_uint4(n_in, n_on, n_through, n_occluded);
    } else {
        out[0] = n_in; out[1] = n_on; out[2] = n_through; out[3] = n_occluded;
    }
    first[i] = f_on;
}

static int cloud_visibility(const float* d_points, int32_t stride, int64_t n, const float* d_depth, const float* d_cam_from_cloud, int32_t n_frames,
                            int32_t height, int32_t width, float fx, float fy, float cx, float cy, float near_z, float far_z, float tol_abs,
                            float tol_rel, int32_t frame_base, int32_t accumulate, uint32_t* d_counts, int32_t* d_first, hipStream_t s) {
    if (stride < 3 || n < 0 || n > (int64_t)1 << 30) return MF_EINVAL;
    if (n_frames < 1 || width < 1 || height < 1 || (int64_t)width * height > (int64_t)1 << 24) return MF_EINVAL;
    if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.f || fy == 0.f || !std::isfinite(cx) || !std::isfinite(cy)) return MF_EINVAL;
    if (!std::isfinite(near_z) || !(near_z > 0.f) || !(far_z > near_z)) return MF_EINVAL;          // far_z: FLT_MAX and +inf mean no limit
    if (!std::isfinite(tol_abs) || !std::isfinite(tol_rel) || tol_abs < 0.f || tol_rel < 0.f) return MF_EINVAL;
    if (frame_base < 0) return MF_EINVAL;
    if (n == 0) return MF_OK;
    if (!d_points || !d_depth || !d_cam_from_cloud || !d_counts || !d_first) return MF_EINVAL;
    VisArgs a;
    a.n = n; a.stride = stride; a.n_frames = n_frames; a.H = height; a.W = width;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.near_z = near_z; a.far_z = far_z; a.tol_abs = tol_abs; a.tol_rel = tol_rel;
    a.frame_base = frame_base; a.accumulate = accumulate != 0;
    a.rows16 = ((uintptr_t)d_counts & 15u) == 0;
    const unsigned blocks = (unsigned)((n + kVisThreads - 1) / kVisThreads);                       // at most 2^22
    hipLaunchKernelGGL(k_cloud_visibility, dim3(blocks), dim3(kVisThreads), 0, s, d_points, d_depth, d_cam_from_cloud, d_counts, d_first, a);
    return hipGetLastError() == hipSuccess ? MF_OK : MF_EHIP;
}

}  // namespace mf

using namespace mf;

extern "C" int mf_cloud_visibility_dev(const float* d_points, int32_t stride, int64_t n, const float* d_depth, const float* d_cam_from_cloud,
                                       int32_t n_frames, int32_t height, int32_t width, float fx, float fy, float cx, float cy, float near_z,
                                       float far_z, float tol_abs, float tol_rel, int32_t frame_base, int32_t accumulate, uint32_t* d_counts,
                                       int32_t* d_first, void* stream) {
    return cloud_visibility(d_points, stride, n, d_depth, d_cam_from_cloud, n_frames, height, width, fx, fy, cx, cy, near_z, far_z, tol_abs, tol_rel,
                            frame_base, accumulate, d_counts, d_first, (hipStream_t)stream);
}
