// mf_eval_image.hip -- run evaluation on images: the segmentation scores, region and boundary counts of two label streams
// (mf_label_confusion_dev, mf_label_boundary_dev), and the view scores, the map's render against the input frame (mf_view_score_dev).  No
// upstream twin: the reference writes its masks and renders and leaves their evaluation to outside tools.  The clouds' half of the
// evaluation is mf_eval.hip; the two share nothing but the compile flag below.
//
// Shape, all three kernels: one workgroup per chunk or tile of ONE frame, the frame's bytes staged in LDS, integer counters in LDS and one
// global atomic per non-zero counter.  Everything that is summed is an integer, so no result depends on the order of execution.  The view
// scores' fp64 arithmetic is rounded operation by operation in the order the header gives: this file is compiled without contraction
// (-ffp-contract=off, and the pragma for a build that forgets the flag).
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/maskfusion_amd.h"
#include "mf_internal.h"

namespace mf {

// ---------------- segmentation scores (mf_label_confusion_dev, mf_label_boundary_dev; DESIGN.md "Segmentation evaluation") ----------------
// Two label streams uint8 [n_frames][H][W]; a 256-entry table per stream maps a raw value to a compact class (< 64) or to kLabVoid.  The
// tables (and the boundary pass's pairing) travel BY VALUE in the kernel's argument block; the first thing a workgroup does is to copy
// them to LDS, where the per-pixel lookups go.  Every counter is an integer: the results do not depend on the order of execution.
constexpr int kLabMaxClasses = 64;
constexpr unsigned kLabVoid = 255u;          // a table entry: the raw value belongs to no class
constexpr unsigned kLabOutside = 254u;       // boundary pass, in LDS only: a position outside the image
constexpr int kLabThreads = 256;

// ---- region counts ----
// One workgroup takes one chunk of kConfChunk pixels of ONE frame (the last chunk of a frame is short), so a workgroup never spans two frames:
// histogram [n_gt][n_est] in LDS, non-zero bins flushed with one global atomic each.  A lane reads 16 pixels of either stream with one 16-byte
// load and adds runs of equal (gt, est) pairs with one LDS atomic per run -- label images are piecewise constant, and without this the 64
// lanes of a wavefront serialise on the background's bin.  A frame need not start at a multiple of 16 bytes (W H odd, a view into a larger
// buffer): the wide loads cover the 16-byte-aligned middle of the chunk when both streams are misaligned by the same amount, the pixels before
// and after it are read byte by byte; when the two misalignments differ, the whole chunk is.
constexpr int kConfChunk = 32768;
struct ConfArgs {
    const uint8_t* est; const uint8_t* gt;
    unsigned* counts;                         // [n_frames][n_gt][n_est]
    int P;                                    // W H
    int chunks;                               // per frame
    int n_est, n_gt;
    uint8_t lut_est[256], lut_gt[256];
};
__device__ __forceinline__ unsigned conf_key(const uint8_t* s_le, const uint8_t* s_lg, unsigned e, unsigned g, int n_est) {
    const unsigned ce = s_le[e], cg = s_lg[g];
    return (ce == kLabVoid || cg == kLabVoid) ? 0xFFFFFFFFu : cg * (unsigned)n_est + ce;
}
__device__ __forceinline__ void conf_flush(unsigned* s_hist, unsigned key, unsigned n) {
    if (key != 0xFFFFFFFFu && n) atomicAdd(&s_hist[key], n);
}
__device__ __forceinline__ void conf_add(unsigned* s_hist, unsigned key, unsigned n, unsigned& cur, unsigned& run) {
    if (key == cur) { run += n; return; }
    conf_flush(s_hist, cur, run);
    cur = key; run = n;
}
__global__ __launch_bounds__(kLabThreads) void k_label_confusion(ConfArgs a) {
    __shared__ unsigned s_hist[kLabMaxClasses * kLabMaxClasses];
    __shared__ uint8_t s_le[256], s_lg[256];
    const int tid = threadIdx.x;
    const int frame = blockIdx.x / a.chunks, chunk = blockIdx.x - frame * a.chunks;
    const int bins = a.n_gt * a.n_est;
    s_le[tid] = a.lut_est[tid];
    s_lg[tid] = a.lut_gt[tid];
    for (int b = tid; b < bins; b += kLabThreads) s_hist[b] = 0u;
    __syncthreads();
    const uint8_t* pe = a.est + (size_t)frame * a.P;
    const uint8_t* pg = a.gt + (size_t)frame * a.P;
    const int beg = chunk * kConfChunk, end = min(a.P, beg + kConfChunk);
    // [v0, v1): whole 16-byte groups at 16-byte-aligned addresses of both streams
    const unsigned me = (unsigned)(((uintptr_t)pe + (unsigned)beg) & 15u), mg = (unsigned)(((uintptr_t)pg + (unsigned)beg) & 15u);
    int v0 = end, v1 = end;
    if (me == mg) {
        v0 = min(end, beg + (int)((16u - me) & 15u));
        v1 = v0 + ((end - v0) & ~15);
    }
    unsigned cur = 0xFFFFFFFFu, run = 0u;
    for (int i = v0 + tid * 16; i < v1; i += kLabThreads * 16) {
        const uint4 e4 = *(const uint4*)(pe + i), g4 = *(const uint4*)(pg + i);
        const unsigned ew[4] = {e4.x, e4.y, e4.z, e4.w}, gw[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned e = ew[w], g = gw[w];
            if (e == (e & 255u) * 0x01010101u && g == (g & 255u) * 0x01010101u) {   // four equal pixels: one lookup
                conf_add(s_hist, conf_key(s_le, s_lg, e & 255u, g & 255u, a.n_est), 4u, cur, run);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    conf_add(s_hist, conf_key(s_le, s_lg, (e >> (8 * k)) & 255u, (g >> (8 * k)) & 255u, a.n_est), 1u, cur, run);
            }
        }
    }
    conf_flush(s_hist, cur, run);
    // the pixels before and after the aligned middle (at most 15 each), or the whole chunk
    const int head = v0 - beg, rest = head + (end - v1);
    for (int k = tid; k < rest; k += kLabThreads) {
        const int i = k < head ? beg + k : v1 + (k - head);
        conf_flush(s_hist, conf_key(s_le, s_lg, pe[i], pg[i], a.n_est), 1u);
    }
    __syncthreads();
    unsigned* out = a.counts + (size_t)frame * bins;
    for (int b = tid; b < bins; b += kLabThreads) {
        const unsigned v = s_hist[b];
        if (v) atomicAdd(&out[b], v);
    }
}

// ---- boundary counts ----
// One workgroup per tile of kBndTW x kBndTH pixels of one frame.  h = radius + 1.
//   1. the compact labels of the tile and a halo of h pixels -> LDS, one byte per pixel and stream (kLabOutside beyond the image);
//   2. two boundary planes over the tile and a halo of `radius`: the class whose boundary the pixel is, or kLabVoid for none (a pixel is a
//      boundary pixel of its class k when a 4-neighbour inside the image has another label; void and outside pixels are boundaries of nothing).
//      The boundary pixels INSIDE the tile are appended to a list (one LDS atomic each), so that
//   3. the threads share the boundary pixels evenly: each walks the disc dx^2 + dy^2 <= radius^2 over the OTHER stream's plane, rows in the
//      order 0, -1, +1, -2, ..., and stops at the first hit.  An estimate's boundary pixel of class e serves every ground-truth class g with
//      pair[g] = e (s_gmask[e], one bit per g: the pairing need not be one to one);
//   4. counters [n_gt][4] in LDS, one global atomic per non-zero counter.
constexpr int kBndTW = 64, kBndTH = 32, kBndMaxRadius = 16;
constexpr int kBndLabMax = (kBndTW + 2 * (kBndMaxRadius + 1)) * (kBndTH + 2 * (kBndMaxRadius + 1));   // 98 x 66
constexpr int kBndPlaneMax = (kBndTW + 2 * kBndMaxRadius) * (kBndTH + 2 * kBndMaxRadius);             // 96 x 64
struct BndArgs {
    const uint8_t* est; const uint8_t* gt;
    unsigned* out;                            // [n_frames][n_gt][4]
    int W, H, radius;
    int tiles_x, tiles_y;
    int n_gt;
    uint8_t lut_est[256], lut_gt[256], pair[kLabMaxClasses];
};
// the class whose boundary pixel (x, y) of the label plane is (pitch lp), or kLabVoid
__device__ __forceinline__ unsigned bnd_class(const uint8_t* s_lab, int lp, int x, int y) {
    const uint8_t* p = s_lab + y * lp + x;
    const unsigned k = p[0];
    if (k >= (unsigned)kLabMaxClasses) return kLabVoid;
    const unsigned l = p[-1], r = p[1], u = p[-lp], d = p[lp];
    const bool edge = (l != kLabOutside && l != k) || (r != kLabOutside && r != k) || (u != kLabOutside && u != k) || (d != kLabOutside && d != k);
    return edge ? k : kLabVoid;
}
__global__ __launch_bounds__(kLabThreads) void k_label_boundary(BndArgs a) {
    __shared__ uint8_t s_le[kBndLabMax], s_lg[kBndLabMax];          // compact labels, halo radius + 1
    __shared__ uint8_t s_be[kBndPlaneMax], s_bg[kBndPlaneMax];      // boundary planes, halo radius
    __shared__ uint16_t s_list[2 * kBndTW * kBndTH];                // boundary pixels of the tile: (side << 15) | (ty * kBndTW + tx)
    __shared__ unsigned long long s_gmask[kLabMaxClasses];          // estimate class e -> the g with pair[g] = e
    __shared__ unsigned s_cnt[kLabMaxClasses * 4];
    __shared__ uint8_t s_lut_e[256], s_lut_g[256], s_pair[kLabMaxClasses];
    __shared__ int s_halfw[kBndMaxRadius + 1];                      // |dy| -> the largest dx with dx^2 + dy^2 <= radius^2
    __shared__ unsigned s_n;
    const int tid = threadIdx.x;
    const int R = a.radius, h = R + 1;
    const int tile = blockIdx.x % (a.tiles_x * a.tiles_y), frame = blockIdx.x / (a.tiles_x * a.tiles_y);
    const int x0 = (tile % a.tiles_x) * kBndTW, y0 = (tile / a.tiles_x) * kBndTH;
    const int lp = kBndTW + 2 * h, lrows = kBndTH + 2 * h;          // label planes
    const int bp = kBndTW + 2 * R, brows = kBndTH + 2 * R;          // boundary planes
    s_lut_e[tid] = a.lut_est[tid];
    s_lut_g[tid] = a.lut_gt[tid];
    if (tid < kLabMaxClasses) {
        s_pair[tid] = tid < a.n_gt ? a.pair[tid] : (uint8_t)kLabVoid;
        unsigned long long m = 0ull;
        for (int g = 0; g < a.n_gt; ++g) if (a.pair[g] == tid) m |= 1ull << g;
        s_gmask[tid] = m;
    }
    if (tid <= R) {
        int w = 0;
        while ((w + 1) * (w + 1) + tid * tid <= R * R) ++w;
        s_halfw[tid] = w;
    }
    for (int k = tid; k < a.n_gt * 4; k += kLabThreads) s_cnt[k] = 0u;
    if (tid == 0) s_n = 0u;
    __syncthreads();
    // 1.
    const uint8_t* pe = a.est + (size_t)frame * a.W * a.H;
    const uint8_t* pg = a.gt + (size_t)frame * a.W * a.H;
    for (int k = tid; k < lp * lrows; k += kLabThreads) {
        const int ly = k / lp, lx = k - ly * lp;
        const int x = x0 - h + lx, y = y0 - h + ly;
        unsigned e = kLabOutside, g = kLabOutside;
        if (x >= 0 && x < a.W && y >= 0 && y < a.H) {
            const size_t at = (size_t)y * a.W + x;
            e = s_lut_e[pe[at]];
            g = s_lut_g[pg[at]];
        }
        s_le[k] = (uint8_t)e;
        s_lg[k] = (uint8_t)g;
    }
    __syncthreads();
    // 2.  (plane position (bx, by) is label position (bx + 1, by + 1): never on the label planes' rim)
    for (int k = tid; k < bp * brows; k += kLabThreads) {
        const int by = k / bp, bx = k - by * bp;
        const unsigned ce = bnd_class(s_le, lp, bx + 1, by + 1), cg = bnd_class(s_lg, lp, bx + 1, by + 1);
        s_be[k] = (uint8_t)ce;
        s_bg[k] = (uint8_t)cg;
        const int tx = bx - R, ty = by - R;
        if (tx >= 0 && tx < kBndTW && ty >= 0 && ty < kBndTH) {
            const unsigned id = (unsigned)(ty * kBndTW + tx);
            if (ce != kLabVoid && s_gmask[ce] != 0ull) s_list[atomicAdd(&s_n, 1u)] = (uint16_t)id;
            if (cg != kLabVoid) s_list[atomicAdd(&s_n, 1u)] = (uint16_t)(0x8000u | id);
        }
    }
    __syncthreads();
    // 3.
    const unsigned n = s_n;
    for (unsigned k = tid; k < n; k += kLabThreads) {
        const unsigned item = s_list[k];
        const bool gt_side = (item & 0x8000u) != 0u;
        const int id = (int)(item & 0x7FFFu);
        const int at = (id / kBndTW + R) * bp + (id % kBndTW + R);       // the pixel in the boundary planes
        if (gt_side) {
            const unsigned g = s_bg[at], e = s_pair[g];
            atomicAdd(&s_cnt[g * 4 + 2], 1u);
            if (e == kLabVoid) continue;
            bool hit = false;
            for (int j = 0; j <= 2 * R && !hit; ++j) {
                const int dy = (j & 1) ? -((j + 1) >> 1) : (j >> 1);
                const int w = s_halfw[dy < 0 ? -dy : dy];
                const uint8_t* row = s_be + at + dy * bp;
                for (int dx = -w; dx <= w; ++dx)
                    if (row[dx] == e) { hit = true; break; }
            }
            if (hit) atomicAdd(&s_cnt[g * 4 + 3], 1u);
        } else {
            const unsigned e = s_be[at];
            const unsigned long long want = s_gmask[e];
            unsigned long long found = 0ull;
            for (int j = 0; j <= 2 * R && found != want; ++j) {
                const int dy = (j & 1) ? -((j + 1) >> 1) : (j >> 1);
                const int w = s_halfw[dy < 0 ? -dy : dy];
                const uint8_t* row = s_bg + at + dy * bp;
                for (int dx = -w; dx <= w; ++dx) {
                    const unsigned g = row[dx];
                    if (g != kLabVoid) found |= (1ull << g) & want;
                }
            }
            for (unsigned long long m = want; m; m &= m - 1) {
                const int g = __ffsll(m) - 1;
                atomicAdd(&s_cnt[g * 4 + 0], 1u);
                if ((found >> g) & 1ull) atomicAdd(&s_cnt[g * 4 + 1], 1u);
            }
        }
    }
    __syncthreads();
    // 4.
    unsigned* out = a.out + (size_t)frame * a.n_gt * 4;
    for (int k = tid; k < a.n_gt * 4; k += kLabThreads) {
        const unsigned v = s_cnt[k];
        if (v) atomicAdd(&out[k], v);
    }
}

// the checks the two calls share; the frame's pixel count -> *P
static int lab_check(const uint8_t* d_est, const uint8_t* d_gt, const void* d_out, int32_t n_frames, int32_t height, int32_t width,
                     const uint8_t* lut_est, int32_t n_est, const uint8_t* lut_gt, int32_t n_gt, int64_t* P) {
    if (!d_est || !d_gt || !d_out || !lut_est || !lut_gt) return MF_EINVAL;
    if (width < 1 || height < 1 || n_frames < 1) return MF_EINVAL;
    if (n_est < 1 || n_est > kLabMaxClasses || n_gt < 1 || n_gt > kLabMaxClasses) return MF_EINVAL;
    *P = (int64_t)width * height;
    if (*P > (int64_t)1 << 30) return MF_EINVAL;                      // (a frame's counters and indices stay within 32 bits)
    for (int v = 0; v < 256; ++v)
        if ((lut_est[v] >= n_est && lut_est[v] != kLabVoid) || (lut_gt[v] >= n_gt && lut_gt[v] != kLabVoid)) return MF_EINVAL;
    return MF_OK;
}

static int label_confusion(const uint8_t* d_est, const uint8_t* d_gt, int32_t n_frames, int32_t height, int32_t width, const uint8_t* lut_est,
                           int32_t n_est, const uint8_t* lut_gt, int32_t n_gt, uint32_t* d_counts, hipStream_t s) {
    int64_t P = 0;
    const int rc = lab_check(d_est, d_gt, d_counts, n_frames, height, width, lut_est, n_est, lut_gt, n_gt, &P);
    if (rc != MF_OK) return rc;
    ConfArgs a;
    memset(&a, 0, sizeof(a));
    a.est = d_est; a.gt = d_gt; a.counts = d_counts; a.P = (int)P; a.n_est = n_est; a.n_gt = n_gt;
    a.chunks = (int)((P + kConfChunk - 1) / kConfChunk);
    memcpy(a.lut_est, lut_est, 256);
    memcpy(a.lut_gt, lut_gt, 256);
    const int64_t blocks = (int64_t)n_frames * a.chunks;
    if (blocks > 0x7FFFFFFF) return MF_EINVAL;
    if (hipMemsetAsync(d_counts, 0, (size_t)n_frames * n_gt * n_est * sizeof(uint32_t), s) != hipSuccess) return MF_EHIP;
    hipLaunchKernelGGL(k_label_confusion, dim3((unsigned)blocks), dim3(kLabThreads), 0, s, a);
    return hipGetLastError() == hipSuccess ? MF_OK : MF_EHIP;
}

static int label_boundary(const uint8_t* d_est, const uint8_t* d_gt, int32_t n_frames, int32_t height, int32_t width, const uint8_t* lut_est,
                          int32_t n_est, const uint8_t* lut_gt, int32_t n_gt, const uint8_t* pair, int32_t radius, uint32_t* d_out, hipStream_t s) {
    int64_t P = 0;
    const int rc = lab_check(d_est, d_gt, d_out, n_frames, height, width, lut_est, n_est, lut_gt, n_gt, &P);
    if (rc != MF_OK) return rc;
    if (!pair || radius < 0 || radius > kBndMaxRadius) return MF_EINVAL;
    for (int g = 0; g < n_gt; ++g)
        if (pair[g] >= n_est && pair[g] != kLabVoid) return MF_EINVAL;
    BndArgs a;
    memset(&a, 0, sizeof(a));
    a.est = d_est; a.gt = d_gt; a.out = d_out; a.W = width; a.H = height; a.radius = radius; a.n_gt = n_gt;
    a.tiles_x = (width + kBndTW - 1) / kBndTW;
    a.tiles_y = (height + kBndTH - 1) / kBndTH;
    memcpy(a.lut_est, lut_est, 256);
    memcpy(a.lut_gt, lut_gt, 256);
    memset(a.pair, (int)kLabVoid, sizeof(a.pair));
    memcpy(a.pair, pair, (size_t)n_gt);
    const int64_t blocks = (int64_t)n_frames * a.tiles_x * a.tiles_y;
    if (blocks > 0x7FFFFFFF) return MF_EINVAL;
    if (hipMemsetAsync(d_out, 0, (size_t)n_frames * n_gt * 4 * sizeof(uint32_t), s) != hipSuccess) return MF_EHIP;
    hipLaunchKernelGGL(k_label_boundary, dim3((unsigned)blocks), dim3(kLabThreads), 0, s, a);
    return hipGetLastError() == hipSuccess ? MF_OK : MF_EHIP;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// view scores: the map's render against the input frame (mf_view_score_dev; DESIGN.md "View evaluation")
// ------------------------------------------------------------------------------------------------------------------------------------
// One workgroup per tile of kViewTW x kViewTH pixels of one frame; thread (tx, ty0) owns the tile's pixels (tx, ty0) and (tx, ty0 + 8).
//   1. the R, G, B bytes of both images over the tile and a halo of 5 -> LDS, one plane per channel and image (0 beyond the image: such a
//      position only enters windows that do not lie wholly inside the image, and those are not counted);
//   2. the counters that need no window (0..8) of the thread's pixels into registers: depths and group from global memory, bytes from LDS;
//   3. per channel: the row pass -- the five quantities x, y, xx, xy, yy filtered along the row for every row of the tile and its halo --
//      into LDS as fp64, then the column pass of the thread's pixels from it; the channel's SSIM value is added to the pixel's sum;
//   4. the pixel's counters -> the group's ten 64-bit counters in LDS (a thread whose two pixels share a group adds them once), and one
//      global 64-bit atomic per non-zero counter.
// Everything that is summed is an integer, so the result does not depend on the order of execution; the fp64 arithmetic is rounded
// operation by operation (no contraction in this file) in the order the header gives.
constexpr int kViewTW = 32, kViewTH = 16, kViewHalo = 5, kViewTaps = 2 * kViewHalo + 1;
constexpr int kViewThreads = 256;
constexpr int kViewPW = kViewTW + 2 * kViewHalo, kViewPH = kViewTH + 2 * kViewHalo;     // the staged planes: 42 x 26
constexpr int kViewMaxGroups = 64, kViewCounters = 10;
constexpr double kViewFix = 16777216.0;      // 2^24: the fixed point of counters 5 and 9
static_assert(kViewTW * kViewTH == 2 * kViewThreads && kViewThreads / kViewTW * 2 == kViewTH, "a thread owns two pixels, 8 rows apart");
struct ViewArgs {
    const uint8_t* render; const float* render_depth;     // [n_frames][H][W][4], [n_frames][H][W]
    const uint8_t* rgb; const float* depth;               // [n_frames][H][W][3], [n_frames][H][W]
    const uint8_t* group;                                 // [n_frames][H][W] or null
    unsigned long long* counts;                           // [n_frames][n_groups][10]
    int W, H, tiles_x, tiles_y, n_groups;
    float max_depth, tau;
    double w[kViewTaps];
};
__device__ __forceinline__ bool view_depth_ok(float z) { return z - z == 0.f && z > 0.f; }   // finite and positive
__global__ __launch_bounds__(kViewThreads) void k_view_score(ViewArgs a) {
    __shared__ uint8_t s_x[3][kViewPW * kViewPH], s_y[3][kViewPW * kViewPH];      // render, input
    __shared__ double s_row[5][kViewPH * kViewTW];
    __shared__ unsigned long long s_cnt[kViewMaxGroups * kViewCounters];
    const int tid = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const int frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
    const int x0 = (tile % a.tiles_x) * kViewTW, y0 = (tile / a.tiles_x) * kViewTH;
    const size_t P = (size_t)a.W * a.H, fbase = (size_t)frame * P;
    for (int k = tid; k < a.n_groups * kViewCounters; k += kViewThreads) s_cnt[k] = 0ull;
    // 1.
    for (int k = tid; k < kViewPW * kViewPH; k += kViewThreads) {
        const int ly = k / kViewPW, lx = k - ly * kViewPW;
        const int x = x0 - kViewHalo + lx, y = y0 - kViewHalo + ly;
        unsigned r[3] = {0u, 0u, 0u}, i[3] = {0u, 0u, 0u};
        if (x >= 0 && x < a.W && y >= 0 && y < a.H) {
            const size_t at = fbase + (size_t)y * a.W + x;
            const uint8_t* pr = a.render + at * 4;
            const uint8_t* pi = a.rgb + at * 3;
            r[0] = pr[0]; r[1] = pr[1]; r[2] = pr[2];
            i[0] = pi[0]; i[1] = pi[1]; i[2] = pi[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { s_x[c][k] = (uint8_t)r[c]; s_y[c][k] = (uint8_t)i[c]; }
    }
    __syncthreads();
    // 2.
    const int tx = tid & (kViewTW - 1), ty0 = tid / kViewTW;
    const int x = x0 + tx;
    int grp[2];                                   // -1: outside the image, or void
    bool window[2];                               // the 11 x 11 window lies inside the image
    unsigned long long cnt[2][kViewCounters - 1]; // counters 0..8 of the two pixels
    double ssum[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int y = y0 + ty0 + j * (kViewTH / 2);
        grp[j] = -1; window[j] = false;
#pragma unroll
        for (int q = 0; q < kViewCounters - 1; ++q) cnt[j][q] = 0ull;
        if (x >= a.W || y >= a.H) continue;
        const size_t at = fbase + (size_t)y * a.W + x;
        const int g = a.group ? (int)a.group[at] : 0;
        if (g >= a.n_groups) continue;
        grp[j] = g;
        const float zr = a.render_depth[at], zi = a.depth[at];
        const bool covered = view_depth_ok(zr), valid = view_depth_ok(zi) && zi <= a.max_depth;
        cnt[j][0] = 1ull; cnt[j][1] = covered ? 1ull : 0ull; cnt[j][2] = valid ? 1ull : 0ull;
        if (covered && valid) {
            const float dz = fabsf(zr - zi);
            cnt[j][3] = 1ull;
            cnt[j][4] = dz <= a.tau ? 1ull : 0ull;
            cnt[j][5] = (unsigned long long)llrint((double)dz * kViewFix);
        }
        const int lk = (ty0 + j * (kViewTH / 2) + kViewHalo) * kViewPW + tx + kViewHalo;
        unsigned sq = 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) { const int d = (int)s_x[c][lk] - (int)s_y[c][lk]; sq += (unsigned)(d * d); }
        cnt[j][6] = sq; cnt[j][7] = covered ? sq : 0u;
        window[j] = x >= kViewHalo && x < a.W - kViewHalo && y >= kViewHalo && y < a.H - kViewHalo;
        cnt[j][8] = window[j] ? 1ull : 0ull;
    }
    // 3.
    for (int c = 0; c < 3; ++c) {
        for (int k = tid; k < kViewPH * kViewTW; k += kViewThreads) {
            const int row = k / kViewTW, col = k - row * kViewTW;
            const uint8_t* px = &s_x[c][row * kViewPW + col];
            const uint8_t* py = &s_y[c][row * kViewPW + col];
            double ax = 0.0, ay = 0.0, axx = 0.0, axy = 0.0, ayy = 0.0;
#pragma unroll
            for (int t = 0; t < kViewTaps; ++t) {
                const double xv = (double)px[t], yv = (double)py[t], wt = a.w[t];
                ax = ax + wt * xv;
                ay = ay + wt * yv;
                axx = axx + wt * (xv * xv);
                axy = axy + wt * (xv * yv);
                ayy = ayy + wt * (yv * yv);
            }
            s_row[0][k] = ax; s_row[1][k] = ay; s_row[2][k] = axx; s_row[3][k] = axy; s_row[4][k] = ayy;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!window[j]) continue;
            const int k0 = (ty0 + j * (kViewTH / 2)) * kViewTW + tx;      // the window's first row of the row pass
            double mx = 0.0, my = 0.0, exx = 0.0, exy = 0.0, eyy = 0.0;
#pragma unroll
            for (int t = 0; t < kViewTaps; ++t) {
                const double wt = a.w[t];
                mx = mx + wt * s_row[0][k0 + t * kViewTW];
                my = my + wt * s_row[1][k0 + t * kViewTW];
                exx = exx + wt * s_row[2][k0 + t * kViewTW];
                exy = exy + wt * s_row[3][k0 + t * kViewTW];
                eyy = eyy + wt * s_row[4][k0 + t * kViewTW];
            }
            const double vx = exx - mx * mx, vy = eyy - my * my, cxy = exy - mx * my;
            const double num = (2.0 * mx * my + 6.5025) * (2.0 * cxy + 58.5225);
            const double den = (mx * mx + my * my + 6.5025) * (vx + vy + 58.5225);
            ssum[j] = ssum[j] + num / den;
        }
        __syncthreads();
    }
    // 4.
    long long fix[2] = {0ll, 0ll};
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (window[j]) fix[j] = llrint(ssum[j] / 3.0 * kViewFix);
    if (grp[0] >= 0 && grp[0] == grp[1]) {
#pragma unroll
        for (int q = 0; q < kViewCounters - 1; ++q) cnt[0][q] += cnt[1][q];
        fix[0] += fix[1];
        grp[1] = -1;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (grp[j] < 0) continue;
        unsigned long long* to = s_cnt + grp[j] * kViewCounters;
#pragma unroll
        for (int q = 0; q < kViewCounters - 1; ++q)
            if (cnt[j][q]) atomicAdd(&to[q], cnt[j][q]);
        if (fix[j]) atomicAdd(&to[9], (unsigned long long)fix[j]);
    }
    __syncthreads();
    unsigned long long* out = a.counts + (size_t)frame * a.n_groups * kViewCounters;
    for (int k = tid; k < a.n_groups * kViewCounters; k += kViewThreads) {
        const unsigned long long v = s_cnt[k];
        if (v) atomicAdd(&out[k], v);
    }
}

static int view_score(const uint8_t* d_render_rgba, const float* d_render_depth, const uint8_t* d_rgb, const float* d_depth, const uint8_t* d_group,
                      int32_t n_frames, int32_t height, int32_t width, int32_t n_groups, float max_depth, float tau, uint64_t* d_counts, hipStream_t s) {
    if (!d_render_rgba || !d_render_depth || !d_rgb || !d_depth || !d_counts) return MF_EINVAL;
    if (width < 1 || height < 1 || n_frames < 1 || (int64_t)width * height > (int64_t)1 << 24) return MF_EINVAL;
    if (n_groups < 1 || n_groups > kViewMaxGroups) return MF_EINVAL;
    if (!(max_depth > 0.f) || !(tau >= 0.f) || !std::isfinite(tau)) return MF_EINVAL;
    ViewArgs a;
    memset(&a, 0, sizeof(a));
    a.render = d_render_rgba; a.render_depth = d_render_depth; a.rgb = d_rgb; a.depth = d_depth; a.group = d_group;
    a.counts = reinterpret_cast<unsigned long long*>(d_counts);
    a.W = width; a.H = height; a.n_groups = n_groups; a.max_depth = max_depth; a.tau = tau;
    a.tiles_x = (width + kViewTW - 1) / kViewTW;
    a.tiles_y = (height + kViewTH - 1) / kViewTH;
    double g[kViewTaps], sum = 0.0;
    for (int k = 0; k < kViewTaps; ++k) {
        g[k] = std::exp(-(double)((k - kViewHalo) * (k - kViewHalo)) / 4.5);
        sum = sum + g[k];
    }
    for (int k = 0; k < kViewTaps; ++k) a.w[k] = g[k] / sum;
    const int64_t blocks = (int64_t)n_frames * a.tiles_x * a.tiles_y;
    if (blocks > 0x7FFFFFFF) return MF_EINVAL;
    if (hipMemsetAsync(d_counts, 0, (size_t)n_frames * n_groups * kViewCounters * sizeof(uint64_t), s) != hipSuccess) return MF_EHIP;
    hipLaunchKernelGGL(k_view_score, dim3((unsigned)blocks), dim3(kViewThreads), 0, s, a);
    return hipGetLastError() == hipSuccess ? MF_OK : MF_EHIP;
}

}  // namespace mf

using namespace mf;

extern "C" int mf_label_confusion_dev(const uint8_t* d_est, const uint8_t* d_gt, int32_t n_frames, int32_t height, int32_t width,
                                      const uint8_t* lut_est, int32_t n_est, const uint8_t* lut_gt, int32_t n_gt, uint32_t* d_counts, void* stream) {
    return label_confusion(d_est, d_gt, n_frames, height, width, lut_est, n_est, lut_gt, n_gt, d_counts, (hipStream_t)stream);
}

extern "C" int mf_label_boundary_dev(const uint8_t* d_est, const uint8_t* d_gt, int32_t n_frames, int32_t height, int32_t width,
                                     const uint8_t* lut_est, int32_t n_est, const uint8_t* lut_gt, int32_t n_gt, const uint8_t* pair, int32_t radius,
                                     uint32_t* d_out, void* stream) {
    return label_boundary(d_est, d_gt, n_frames, height, width, lut_est, n_est, lut_gt, n_gt, pair, radius, d_out, (hipStream_t)stream);
}

extern "C" int mf_view_score_dev(const uint8_t* d_render_rgba, const float* d_render_depth, const uint8_t* d_rgb, const float* d_depth,
                                 const uint8_t* d_group, int32_t n_frames, int32_t height, int32_t width, int32_t n_groups, float max_depth, float tau,
                                 uint64_t* d_counts, void* stream) {
    return view_score(d_render_rgba, d_render_depth, d_rgb, d_depth, d_group, n_frames, height, width, n_groups, max_depth, tau, d_counts,
                      (hipStream_t)stream);
}
