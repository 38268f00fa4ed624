// mf_surfel.hip -- surfel map maintenance on plain HBM arrays (no OpenGL, no transform feedback, no textures).
//
// Replaces (reference, relative to /root/reference):
//   first-frame init         Core/Shaders/vertex_feedback.vert/.geom, init_unstable.vert; Core/Model/Model.cpp:240-285
//   index map                Core/Shaders/index_map.vert/.frag; Core/Model/ModelProjection.cpp:100-152
//   data association         Core/Shaders/data.vert/.geom/.frag; Core/Model/Model.cpp:466-581
//   surfel update            Core/Shaders/update.vert; Core/Model/Model.cpp:583-646
//   clean / append / decay   Core/Shaders/copy_unstable.vert:53-157, .geom; Core/Model/Model.cpp:649-772
//   splat prediction         Core/Shaders/splat.vert, combo_splat.frag; Core/Model/ModelProjection.cpp:187-268
//
// Design (MI355X):
//   * surfels are three float4 streams (48 B/surfel, 16 B per lane per stream, fully coalesced), double buffered;
//   * the GL rasteriser + z-buffer becomes a 64-bit atomicMin on (z bits << 32 | surfel index) per pixel followed by
//     a per-pixel resolve that recomputes the attributes of the winner (ties go to the lower index = GL order);
//   * the 453 MB "update map" the reference clears and scatters into every frame becomes one int per surfel that
//     receives atomicMin(column-major candidate index) -- "first writer wins" without ordering the writers;
//   * transform feedback (ordered stream compaction) becomes a fixed-grid two-pass compaction: pass 1 writes keep
//     flags + per-workgroup counts, pass 2 sums the counts of the workgroups before it in its prologue and copies
//     survivors in order with wavefront ballots.  Surfel order is therefore exactly the reference's (old surfels
//     first, then new ones in column-major pixel order), and no workgroup ever spins on another.
//   * every per-surfel grid is fixed-size and bounded by a device-resident count: no host round trip per pass.
// Every float op individually rounded in this file: several passes re-derive the same quantity in different kernels
// (a surfel's camera-space position in the index-map resolve and again in the clean pass) and then compare them for
// strict inequality; with per-kernel FMA contraction those self-comparisons flip at random.  It also keeps these
// kernels within rounding of a plain reading of the shaders (the oracle is built with -ffp-contract=off).
#pragma clang fp contract(off)
#include "mf_device.h"
#include "mf_walk.h"
#include "mf_sprite_device.h"
#include "mf_rgbd_device.h"

namespace mf {

// ------------------------------------------------------------------------------------------------
// fills
// ------------------------------------------------------------------------------------------------
__global__ void k_fill_keys(unsigned long long* keys, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) keys[i] = kEmptyKey;
}
void launch_fill_keys(unsigned long long* keys, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_fill_keys, dim3(min((n + 255) / 256, 2048)), dim3(256), 0, s, keys, n);
}
__global__ void k_fill_int(int* p, int v, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = v;
}
void launch_fill_int(int* p, int v, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_fill_int, dim3(min((n + 255) / 256, 2048)), dim3(256), 0, s, p, v, n);
}

// ------------------------------------------------------------------------------------------------
// ordered compaction machinery (fixed grid of kCompactBlocks workgroups x 256 threads)
// ------------------------------------------------------------------------------------------------
// number of quarter-rate candidate pixels of frame `tick` (data.vert:117): x % 2 == y % 2 == tick % 2
__device__ __forceinline__ int cand_count(int W, int H, int tick) {
    const int par = tick & 1;
    return ((W - par + 1) / 2) * ((H - par + 1) / 2);
}

// (the grid of an ordered-compaction launch is at most kCompactBlocks workgroups -- the size of its count array -- and the host's choice below that:
// compact_blocks_for)
__device__ __forceinline__ int chunk_size(int n) {
    const int blocks = (int)gridDim.x;
    const int c = (n + blocks - 1) / blocks;
    return ((c + 255) / 256) * 256;
}

// sum of 256 per-thread ints -> every thread gets the block total; s_w: 4 ints of LDS
__device__ __forceinline__ int block_sum_i(int v, int* s_w) {
    v = wave_sum_i(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    const int tot = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return tot;
}

// exclusive prefix of block_counts for this workgroup (prologue of pass 2)
__device__ __forceinline__ int block_base(const int* __restrict__ block_counts, int* s_w) {
    int v = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) v += block_counts[b];
    return block_sum_i(v, s_w);
}

// ------------------------------------------------------------------------------------------------
// first-frame initialisation: one record per pixel in column-major slots + keep flag, then compaction
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_init_records(const uint8_t* __restrict__ rgb, const float* __restrict__ depthRaw,
                                                      const float* __restrict__ depthF, int W, int H, Intr k, float maxDepth,
                                                      const FrameDev* __restrict__ frame, float4* __restrict__ rec,
                                                      uint8_t* __restrict__ flags) {
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= W || j >= H) return;
    const int slot = i * H + j;  // FeedbackBuffer.cpp:44-50: column-major vertex order
    const float x = (float)i + 0.5f, y = (float)j + 0.5f;
    const float3 vraw = get_vertex(depthRaw, W, H, i, j, x, y, k);
    if (vraw.z <= 0 || vraw.z > maxDepth) { flags[slot] = 0; return; }
    const float3 vfil = get_vertex(depthF, W, H, i, j, x, y, k);
    const float3 n = get_normal_central(depthF, W, H, i, j, x, y, vfil, k);
    const uint8_t* p = rgb + (size_t)(j * W + i) * 3;
    rec[slot * 3 + 0] = make_float4(vraw.x, vraw.y, vraw.z, surfel_confidence(x, y, 1.0f, k));
    rec[slot * 3 + 1] = make_float4((float)((p[0] << 16) + (p[1] << 8) + p[2]), 0.f, 1.f, (float)frame->tick);
    rec[slot * 3 + 2] = make_float4(n.x, n.y, n.z, surfel_radius(vfil.z, n.z, k));
    flags[slot] = 1;
}

void launch_init_surfels(const uint8_t* rgb, const float* depthRaw, const float* depthF, int W, int H, Intr k, float maxDepth,
                         const FrameDev* frame, float4* rec, uint8_t* flags, hipStream_t s) {
    dim3 grid((W + 63) / 64, (H + 3) / 4);
    hipLaunchKernelGGL(k_init_records, grid, dim3(256), 0, s, rgb, depthRaw, depthF, W, H, k, maxDepth, frame, rec, flags);
}

__global__ __launch_bounds__(256) void k_count_flags(const uint8_t* __restrict__ flags, int n, int* __restrict__ block_counts) {
    __shared__ int s_w[4];
    const int chunk = chunk_size(n);
    const int beg = blockIdx.x * chunk, end = min(n, beg + chunk);
    int v = 0;
    for (int i = beg + threadIdx.x; i < end; i += 256) v += flags[i] ? 1 : 0;
    const int tot = block_sum_i(v, s_w);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_compact_records(const float4* __restrict__ rec, const uint8_t* __restrict__ flags, int n,
                                                         Surfels dst, FrameDev* __restrict__ frame,
                                                         const int* __restrict__ block_counts, int* __restrict__ host_count) {
    __shared__ int s_w[4];
    int base = block_base(block_counts, s_w);
    const int chunk = chunk_size(n);
    const int beg = blockIdx.x * chunk, end = min(n, beg + chunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i0 = beg; i0 < end; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < end && flags[i];
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_w[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += s_w[w];
        const int tot = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (keep) {
            const int o = off + lane_rank(m);
            if (o < dst.cap) { dst.pc[o] = rec[i * 3 + 0]; dst.ct[o] = rec[i * 3 + 1]; dst.nr[o] = rec[i * 3 + 2]; }
        }
        base += tot;
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        frame->count = frame->phys = min(base, dst.cap);   // a dense buffer without a run table
        frame->runs = 0; frame->first = 0; frame->first_run = 0;
        if (host_count) *host_count = min(base, dst.cap);
    }
}

void launch_compact_records(const float4* rec, const uint8_t* flags, int n, Surfels dst, FrameDev* frame, int* block_counts,
                            int* host_count_mirror, hipStream_t s) {
    hipLaunchKernelGGL(k_count_flags, dim3(kCompactBlocks), dim3(256), 0, s, flags, n, block_counts);
    hipLaunchKernelGGL(k_compact_records, dim3(kCompactBlocks), dim3(256), 0, s, rec, flags, n, dst, frame, block_counts,
                       host_count_mirror);
}

// ------------------------------------------------------------------------------------------------
// index map: scatter (z-test as 64-bit atomicMin) + resolve
// Raster rule: a 1-px point lands in texel (floor(u), floor(v)); LESS on z; lower index wins ties.
// ------------------------------------------------------------------------------------------------
// (bodies are __device__ functions: the single-model kernels call them with their own arguments, the batched object-model kernels at the
// end of this file with one model's arguments picked by blockIdx.z)
// One surfel per lane; `live` lanes hold a surfel index i (the others only take part in the wavefront exchange below).
__device__ __forceinline__ void index_scatter_one(const Surfels& src, int i, bool live, float time, const float* Ri, float3 ti, int W, int H, Intr k,
                                                  float maxDepth, int timeDelta, unsigned long long* __restrict__ keys, int transposed,
                                                  bool pretest = false) {
    int p = -1;
    unsigned long long key = kEmptyKey;
    if (live) {
        const float4 pc = src.pc[i];
        const float lastTime = src.ct[i].w;
        const float3 h = mul33(Ri, f3(pc.x, pc.y, pc.z)) + ti;
        if (!(h.z > maxDepth || h.z <= 0 || time - lastTime > (float)timeDelta)) {  // index_map.vert:46
            const float u = ((k.fx * h.x) / h.z) + k.cx;
            const float v = ((k.fy * h.y) / h.z) + k.cy;
            if (u >= 0.f && u < (float)W && v >= 0.f && v < (float)H) {
                // transposed: column-major key image.  Surfels are stored in column-major creation order (data.vert), so the surfels of a wavefront
                // then meet in a few cache lines of keys instead of one line per image row: on the 26.9 M-surfel map of configs[4] the same pass takes
                // 75 us column-major and 133-168 us row-major (profiles/r05_c4_kernel_stats.csv, r05p_c4_kernel_stats.csv), at VGA the copy-update with
                // the scatter riding on it 17.4 against 23.2 us.  (The packed object maps of that scenario, ~85 surfels per pixel, behave the other way
                // round -- 257 against 190 us -- and are scattered row-major.)  The RESOLVE brings the result into the order its consumer reads it in.
                p = transposed ? (int)floorf(u) * H + (int)floorf(v) : (int)floorf(v) * W + (int)floorf(u);
                key = ((unsigned long long)__float_as_uint(h.z) << 32) | (unsigned)i;
            }
        }
    }
    // Neighbouring surfels of a buffer are neighbours in space (creation order), and in a dense map several in a row land on the SAME texel:
    // each lane takes over the smaller key of the lanes 1, 2 and 4 below it that hit its texel, and only the last lane of such a group (of up
    // to eight) goes to memory with the group's minimum -- the z-test is a minimum, so the keys in memory are the same bits, with a fraction of the
    // device-scope atomics (which retire at a few tens of nanoseconds each when they meet on an address).
#pragma unroll
    for (int d = 1; d <= 4; d <<= 1) {
        const int pn = __shfl_up(p, d, 64);
        const unsigned lo = __shfl_up((unsigned)(key & 0xFFFFFFFFull), d, 64), hi = __shfl_up((unsigned)(key >> 32), d, 64);
        const unsigned long long kn = ((unsigned long long)hi << 32) | lo;
        if ((int)(threadIdx.x & 63) >= d && pn == p && kn < key) key = kn;
    }
    // (three steps cover the 7 lanes below: a lane writes when the next lane hits another texel, and every 8th lane writes in any case, so
    // that a longer group is written in pieces none of whose members is lost)
    const int p_next = __shfl_down(p, 1, 64);
    const bool last_of_group = (threadIdx.x & 7) == 7 || p_next != p;
    if (p >= 0 && last_of_group) {
        if (pretest) zmin_key_pretested(&keys[p], key);
        else zmin_key(&keys[p], key);
    }
}

__device__ __forceinline__ void index_scatter_body(Surfels src, const FrameDev* __restrict__ frame,
                                                   const PoseDev* __restrict__ pose, int W, int H, Intr k, float maxDepth,
                                                   int timeDelta, unsigned long long* __restrict__ keys, int transposed,
                                                   const int* __restrict__ vis_list = nullptr, const int* __restrict__ vis_count = nullptr,
                                                   bool pretest = false) {
    const float time = (float)frame->tick;
    float Ri[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Ri[q] = pose->Ri[q];
    const float3 ti = f3(pose->ti[0], pose->ti[1], pose->ti[2]);
    for_each_surfel_slice<1>(src, frame, vis_list, vis_count, [&](int i, bool live) {
        index_scatter_one(src, i, live, time, Ri, ti, W, H, k, maxDepth, timeDelta, keys, transposed, pretest);
    });
}

__global__ __launch_bounds__(256) void k_index_scatter(Surfels src, const FrameDev* __restrict__ frame,
                                                       const PoseDev* __restrict__ pose, int W, int H, Intr k, float maxDepth,
                                                       int timeDelta, unsigned long long* __restrict__ keys, int transposed,
                                                       const int* __restrict__ vis_list, const int* __restrict__ vis_count) {
    index_scatter_body(src, frame, pose, W, H, k, maxDepth, timeDelta, keys, transposed, vis_list, vis_count);
}

void launch_index_scatter(Surfels src, const PassFrame& f, const PassModel& m, hipStream_t s, int blocks, const VisList* vis) {
    hipLaunchKernelGGL(k_index_scatter, dim3(blocks), dim3(256), 0, s, src, m.frame, m.pose, f.W, f.H, f.k, f.maxDepthProcessed, f.timeDelta, m.scr.keys,
                       1, vis ? vis->list : nullptr, vis ? vis->count : nullptr);
}

// ------------------------------------------------------------------------------------------------
// run table (Surfels::box) from scratch, and the visibility test over it
// ------------------------------------------------------------------------------------------------
// what a run's table entry says about its surfels, per thread: box of the positions, newest lastTime, lowest confidence (order-preserving ints),
// and whether one of them carries a time stamp <= 0 (`unstamped`: the age rule of Model::clean treats those apart, k_cull_clean rule (b))
struct RunAcc {
    int lo[3], hi[3], tmax, cmin, unstamped;
    __device__ __forceinline__ void reset() {
        lo[0] = lo[1] = lo[2] = kBoxEmptyMin; hi[0] = hi[1] = hi[2] = kBoxEmptyMax; tmax = kBoxEmptyMax; cmin = kBoxEmptyMin; unstamped = 0;
    }
    __device__ __forceinline__ void add(float4 pc, float lastTime) {
        if (pc.x == pc.x && pc.y == pc.y && pc.z == pc.z) {   // (a NaN position is never in view)
            const int ex = box_enc(pc.x), ey = box_enc(pc.y), ez = box_enc(pc.z);
            lo[0] = min(lo[0], ex); lo[1] = min(lo[1], ey); lo[2] = min(lo[2], ez);
            hi[0] = max(hi[0], ex); hi[1] = max(hi[1], ey); hi[2] = max(hi[2], ez);
        }
        // (a NaN time stamp passes every "seen within timeDelta" test of the passes -- !(time - NaN > delta) -- : such a surfel counts as seen now)
        tmax = max(tmax, lastTime == lastTime ? box_enc(lastTime) : 0x7F800000);
        if (pc.w == pc.w) cmin = min(cmin, box_enc(pc.w));   // (a NaN confidence is below no threshold: the age rule of clean never drops it)
        if (lastTime <= 0.f) unstamped = 1;                  // (false for a NaN stamp: it passes every age test, see above)
    }
};
// block reduction of one run's entry: per-thread (already reduced over the thread's own surfels) -> s_red[wavefront][kRunRed]
constexpr int kRunRed = 9;
__device__ __forceinline__ void run_box_reduce(const RunAcc& t, int (*s_red)[kRunRed]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int lo[3], hi[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { lo[q] = wave_min_i(t.lo[q]); hi[q] = wave_max_i(t.hi[q]); }
    const int tmax = wave_max_i(t.tmax), cmin = wave_min_i(t.cmin);
    const int unstamped = __ballot(t.unstamped != 0) != 0ull ? 1 : 0;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { s_red[wave][q] = lo[q]; s_red[wave][4 + q] = hi[q]; }
        s_red[wave][3] = tmax; s_red[wave][7] = cmin; s_red[wave][8] = unstamped;
    }
}
// one thread: the four wavefronts' partial results -> the table entry of run r (start slot, live surfels)
__device__ __forceinline__ void run_box_store(int4* __restrict__ box, int r, int start, int len, const int (*s_red)[kRunRed]) {
    int4 a, b;
    a.x = min(min(s_red[0][0], s_red[1][0]), min(s_red[2][0], s_red[3][0]));
    a.y = min(min(s_red[0][1], s_red[1][1]), min(s_red[2][1], s_red[3][1]));
    a.z = min(min(s_red[0][2], s_red[1][2]), min(s_red[2][2], s_red[3][2]));
    a.w = max(max(s_red[0][3], s_red[1][3]), max(s_red[2][3], s_red[3][3]));
    b.x = max(max(s_red[0][4], s_red[1][4]), max(s_red[2][4], s_red[3][4]));
    b.y = max(max(s_red[0][5], s_red[1][5]), max(s_red[2][5], s_red[3][5]));
    b.z = max(max(s_red[0][6], s_red[1][6]), max(s_red[2][6], s_red[3][6]));
    b.w = start;
    const int cmin = min(min(s_red[0][7], s_red[1][7]), min(s_red[2][7], s_red[3][7]));
    const int unstamped = s_red[0][8] | s_red[1][8] | s_red[2][8] | s_red[3][8];
    box[kBoxStride * r] = a; box[kBoxStride * r + 1] = b; box[kBoxStride * r + 2] = make_int4(len, cmin, unstamped, 0);
}

// A DENSE buffer (slots [0, count)) gets its table: fixed runs of kRun slots.  refresh != 0: the buffer HAS a table (frame->runs > 0) and only the
// entries' contents are recomputed from the surfels (after an in-place update outside a frame: merged surfels moved, their time stamps changed).
__global__ __launch_bounds__(256) void k_run_table(Surfels s, FrameDev* __restrict__ frame, int refresh) {
    __shared__ int s_red[4][kRunRed];
    const int n = frame->count;
    const int runs = refresh ? frame->runs : (n + kRun - 1) / kRun;
    for (int r = blockIdx.x; r < runs; r += gridDim.x) {
        const int start = refresh ? run_start(s.box, r) : r * kRun, len = refresh ? run_len(s.box, r) : min(n - r * kRun, kRun);
        RunAcc acc;
        acc.reset();
        for (int i = start + (int)threadIdx.x; i < start + len; i += 256) acc.add(s.pc[i], s.ct[i].w);
        run_box_reduce(acc, s_red);
        __syncthreads();
        if (threadIdx.x == 0) run_box_store(s.box, r, start, len, s_red);
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && !refresh) {
        frame->runs = runs; frame->phys = n; frame->first = 0; frame->first_run = 0;
    }
}
void launch_run_table(Surfels s, FrameDev* frame, hipStream_t st, bool refresh) {
    hipLaunchKernelGGL(k_run_table, dim3(1024), dim3(256), 0, st, s, frame, refresh ? 1 : 0);
}
// entries of a buffer's run table: the fixed runs of a full buffer + the runs Model::clean appends, one frame's new surfels after the other
// (<= P / 4 surfels in <= P / (4 kRun) + 1 runs per frame), until the host compacts the buffer (mf_frame.inl: runs_ub)
size_t run_table_runs(long capacity, long pixels) { return (size_t)(2 * ((capacity + kRun - 1) / kRun) + 4 * ((pixels / 4 + kRun - 1) / kRun + 2) + 64); }
size_t run_table_entries(long capacity, long pixels) { return (size_t)kBoxStride * run_table_runs(capacity, pixels); }

// every corner of a run's box outside the SAME half-space => the whole box is: near / far, then the four image sides as planes through the eye
// (u < -2  <=>  fx x + (cx + 2) z < 0 for z > 0).  The per-surfel tests of the passes are u in [0, W] x [0, H] and 0 <= z <= maxDepth on individually
// rounded floats: the box is tested against the image grown by 2 px and the depth range grown by 1 cm -- metres against rounding errors of
// micrometres.  zlo / zhi: the depth range of the box's corners in the camera frame.
// outside (optional): bit q set = the whole box lies outside the image on side q (0 left, 1 right, 2 top, 3 bottom)
__device__ __forceinline__ bool run_box_in_frustum(int4 a, int4 b, const PoseDev* __restrict__ pose, int W, int H, Intr k, float maxDepth, float& zlo, float& zhi,
                                                   int* outside = nullptr) {
    const float lo[3] = {box_dec(a.x), box_dec(a.y), box_dec(a.z)}, hi[3] = {box_dec(b.x), box_dec(b.y), box_dec(b.z)};
    int out_near = 1, out_far = 1, out_l = 1, out_r = 1, out_t = 1, out_b = 1;
    zlo = INFINITY; zhi = -INFINITY;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float3 p = f3((c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]);
        const float3 h = mul33(pose->Ri, p) + f3(pose->ti[0], pose->ti[1], pose->ti[2]);
        zlo = fminf(zlo, h.z); zhi = fmaxf(zhi, h.z);
        out_near &= h.z < -0.01f;
        out_far &= h.z > maxDepth + 0.01f;
        out_l &= k.fx * h.x + (k.cx + 2.f) * h.z < 0.f;
        out_r &= k.fx * h.x + (k.cx - (float)W - 2.f) * h.z > 0.f;
        out_t &= k.fy * h.y + (k.cy + 2.f) * h.z < 0.f;
        out_b &= k.fy * h.y + (k.cy - (float)H - 2.f) * h.z > 0.f;
    }
    if (outside) *outside = out_l | (out_r << 1) | (out_t << 2) | (out_b << 3);
    return !(out_near | out_far | out_l | out_r | out_t | out_b);
}
// the listed runs go to `list` in no particular order; the last workgroup to finish publishes their number and re-arms the counters
__device__ __forceinline__ void run_list_append(bool listed, int r, int* __restrict__ list, int* __restrict__ count, int* __restrict__ ctl) {
    const unsigned long long m = __ballot(listed);
    int base = 0;
    if ((threadIdx.x & 63) == 0 && m) base = atomicAdd(&ctl[0], __popcll(m));
    base = __shfl(base, 0, 64);
    if (listed) list[base + lane_rank(m)] = r;
}
__device__ __forceinline__ bool run_list_finish(int* __restrict__ count, int* __restrict__ ctl) {
    __syncthreads();
    if (threadIdx.x != 0) return false;
    // (every workgroup's slot reservations have returned before its barrier: relaxed atomics suffice, an agent-scope release would write the L2 back)
    const int done = atomicAdd(&ctl[1], 1);
    if (done != (int)gridDim.x - 1) return false;
    count[0] = __hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ctl[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ctl[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// One thread per run: conservative frustum test of the run's box under `pose` and the activity test (no surfel seen within timeDelta: every
// projection pass drops all of them, index_map.vert:46, splat.vert:58).
__global__ __launch_bounds__(256) void k_cull(Surfels s, const FrameDev* __restrict__ frame, const PoseDev* __restrict__ pose, int W, int H, Intr k,
                                              float maxDepth, int timeDelta, int* __restrict__ list, int* __restrict__ count, int* __restrict__ ctl) {
    const int runs = frame->runs;
    const float time = (float)frame->tick;
    const int r = blockIdx.x * 256 + threadIdx.x;
    bool vis = false;
    if (r < runs) {
        const int4 a = s.box[kBoxStride * r], b = s.box[kBoxStride * r + 1];
        if (run_len(s.box, r) > 0 && a.x <= b.x && a.y <= b.y && a.z <= b.z && !(time - box_dec(a.w) > (float)timeDelta)) {
            float zlo, zhi;
            vis = run_box_in_frustum(a, b, pose, W, H, k, maxDepth, zlo, zhi);
        }
    }
    run_list_append(vis, r, list, count, ctl);
    (void)run_list_finish(count, ctl);
}
void launch_cull(Surfels s, const FrameDev* frame, const PoseDev* pose, int W, int H, Intr k, float maxDepth, int timeDelta, int* list, int* count,
                 int* ctl, int max_runs, hipStream_t st) {
    hipLaunchKernelGGL(k_cull, dim3((max_runs + 255) / 256), dim3(256), 0, st, s, frame, pose, W, H, k, maxDepth, timeDelta, list, count, ctl);
}

// Two consumers, two output shapes (the index_map.frag attachments that each of them samples):
//   packed == nullptr (the pass that feeds fuse): index + vertConf + normRad as separate images;
//   packed != nullptr (the pass that feeds clean): ONE 32 B record per texel {vertConf.xyzw | colorTime.z, colorTime.w,
//     index bits, 0} -- clean gathers 9 texels per surfel, and three separate images cost it three cache lines per tap.
// Resolve: the winning surfel of every texel -> the maps the consumer reads.  Two consumers, two orders: data.vert's window (fuse_data) reads
// {index, vertConf, normRad(, colorTime)} row-major; copy_unstable.vert's window (clean) reads the packed map {position, confidence | initTime,
// lastTime, index, 0} COLUMN-major (surfels are stored in column-major creation order: consecutive surfels then read consecutive texels).  The
// key image comes in either order too (index_scatter_one).  Where the two orders agree a thread handles texel p of both; where they differ a
// workgroup handles a 16 x 16-pixel tile and transposes it through the LDS: keys are read and records written in pieces of 128-512 bytes.
// Every form also resets the key it read (ready for the next scatter: saves a separate clear pass).
struct ResolvedTexel { int index; float4 vc, nr, ct, p0, p1; };
// The 16-byte tap of the pass that feeds clean ("cleanTap16"): clean_test's window uses a tap only through x, y, z, initTime, "live" (index > 0,
// confidence above the model's threshold, z > 0 -- both counting rules hold `idx > 0 && v.w > thr && v.z > lp.z` under lp.z > 0) and "updated in
// this frame" (lastTime == tick).  One float4 {x, y, z', initTime}: z' = NaN for a tap that is not live, else z with the sign bit = updated.
struct Tap16 { float thr, time; };     // the model's confidence threshold, (float)frame->tick -- the values the clean pass of the same enqueue tests with
__device__ __forceinline__ float4 tap16_encode(float3 h, float conf, float initTime, float lastTime, int id, Tap16 t) {
    const bool live = id > 0 && conf > t.thr && h.z > 0;
    return make_float4(h.x, h.y, live ? (lastTime == t.time ? -h.z : h.z) : __int_as_float(0x7fc00000), initTime);
}
template <bool kPacked>
__device__ __forceinline__ ResolvedTexel resolve_texel(const Surfels& src, const PoseDev* __restrict__ pose, unsigned long long key, bool want_ct, int first,
                                                       const Tap16* tap16 = nullptr) {
    ResolvedTexel r;
    r.index = 0;
    r.vc = r.nr = r.ct = r.p0 = r.p1 = make_float4(0, 0, 0, 0);
    if (kPacked && tap16) r.p0.z = __int_as_float(0x7fc00000);    // an empty texel is no live tap
    if (key == kEmptyKey) return r;
    const int i = (int)(unsigned)(key & 0xFFFFFFFFull);
    // The index image holds the VERTEX ID of the winner (index_map.frag), and vertex 0 -- the first surfel of the buffer -- cannot be told from
    // the cleared texture: it occludes like any other surfel and is then read as "no surfel" (data.vert, copy_unstable.vert test index > 0).  In a
    // sparse buffer the first surfel is slot frame->first.
    const int id = i == first ? 0 : i;
    const float4 pc = src.pc[i];
    const float3 h = mul33(pose->Ri, f3(pc.x, pc.y, pc.z)) + f3(pose->ti[0], pose->ti[1], pose->ti[2]);
    if (kPacked) {
        const float4 c4 = src.ct[i];
        r.p0 = tap16 ? tap16_encode(h, pc.w, c4.z, c4.w, id, *tap16) : make_float4(h.x, h.y, h.z, pc.w);
        r.p1 = make_float4(c4.z, c4.w, __int_as_float(id), 0.f);
    } else {
        const float4 n4 = src.nr[i];
        const float3 n = normalize_gl(mul33(pose->Ri, f3(n4.x, n4.y, n4.z)));
        r.index = id;
        r.vc = make_float4(h.x, h.y, h.z, pc.w);
        r.nr = make_float4(n.x, n.y, n.z, n4.w);
        if (want_ct) r.ct = src.ct[i];   // colorTime image: only the clean pass of a freshly spawned model reads it from here
    }
    return r;
}
// a workgroup's texels -> the decay statistics (one atomic per statistic and wavefront that saw such a texel)
__device__ __forceinline__ void decay_stats_add(const ResolveOut& o, bool in_image, int x, int y, int W, int H, float depth, int maskValue) {
    if (!o.decay_stats) return;
    const bool foreign = in_image && maskValue != o.maskID && maskValue < 255 && depth == depth;
    const int e = box_enc(depth);
    const bool side[4] = {foreign && x == 0, foreign && x == W - 1, foreign && y == 0, foreign && y == H - 1};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (__ballot(side[q]) == 0ull) continue;      // (wavefront-uniform: most wavefronts hold no border texel at all)
        const int lo = wave_min_i(side[q] ? e : kBoxEmptyMin), hi = wave_max_i(side[q] ? e : kBoxEmptyMax);
        if ((threadIdx.x & 63) == 0) { atomicMin(&o.decay_stats[2 * q], lo); atomicMax(&o.decay_stats[2 * q + 1], hi); }
    }
    if (__ballot(foreign) != 0ull) {
        const int amin = wave_min_i(foreign ? e : kBoxEmptyMin);
        if ((threadIdx.x & 63) == 0) atomicMin(&o.decay_stats[8], amin);
    }
}
// row-major keys -> row-major maps: texel p of the key image is texel p of the outputs
template <bool kPacked>
__device__ __forceinline__ void index_resolve_same_body(Surfels src, const PoseDev* __restrict__ pose, unsigned long long* __restrict__ keys, int P, ResolveOut o) {
    static_assert(!kPacked, "the packed map goes through a tile kernel");
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const unsigned long long key = keys[p];
    keys[p] = kEmptyKey;
    const ResolvedTexel r = resolve_texel<false>(src, pose, key, o.ct != nullptr, o.frame->first);
    o.index[p] = r.index; o.vc[p] = r.vc; o.nr[p] = r.nr;
    if (o.ct) o.ct[p] = r.ct;
}
// keys and outputs in different orders (column-major keys -> row-major maps, row-major keys -> column-major packed map): one tile per workgroup
constexpr int kResolveTile = 16;
template <bool kPacked>
__device__ __forceinline__ void index_resolve_transposing_body(Surfels src, const PoseDev* __restrict__ pose, unsigned long long* __restrict__ keys, int W, int H,
                                                               ResolveOut o, int tile) {
    __shared__ float4 s_a[kResolveTile][kResolveTile + 1], s_b[kResolveTile][kResolveTile + 1], s_c[kPacked ? 1 : kResolveTile][kResolveTile + 1];
    __shared__ int s_i[kPacked ? 1 : kResolveTile][kResolveTile + 1];
    __shared__ uint8_t s_mk[kPacked ? kResolveTile : 1][kResolveTile + 1];
    const int tilesX = (W + kResolveTile - 1) / kResolveTile;
    const int x0 = (tile % tilesX) * kResolveTile, y0 = (tile / tilesX) * kResolveTile;
    const int f = threadIdx.x & (kResolveTile - 1), g = threadIdx.x / kResolveTile;   // f: the fast coordinate of consecutive lanes
    {   // read the keys in THEIR order: packed output <- row-major keys (x fast), maps <- column-major keys (y fast)
        const int lx = kPacked ? f : g, ly = kPacked ? g : f;
        const int x = x0 + lx, y = y0 + ly;
        const Tap16 t16{o.tapThreshold, (float)o.frame->tick};
        const Tap16* tap = (kPacked && o.tap16) ? &t16 : nullptr;
        ResolvedTexel r = resolve_texel<kPacked>(src, pose, kEmptyKey, false, 0, tap);
        int mk = 0;
        if (x < W && y < H) {
            const int p = kPacked ? y * W + x : x * H + y;
            const unsigned long long key = keys[p];
            keys[p] = kEmptyKey;
            r = resolve_texel<kPacked>(src, pose, key, o.ct != nullptr, o.frame->first, tap);
            if (kPacked && o.maskT) { r.p1.w = o.depthF[p]; mk = o.mask[p]; s_mk[lx][ly] = (uint8_t)mk; }
        }
        if (kPacked && o.maskT) decay_stats_add(o, x < W && y < H, x, y, W, H, r.p1.w, mk);
        if (kPacked) { s_a[lx][ly] = r.p0; s_b[lx][ly] = r.p1; }
        else { s_i[lx][ly] = r.index; s_a[lx][ly] = r.vc; s_b[lx][ly] = r.nr; if (o.ct) s_c[lx][ly] = r.ct; }
    }
    __syncthreads();
    {   // write the outputs in THEIR order: packed column-major (y fast), maps row-major (x fast)
        const int lx = kPacked ? g : f, ly = kPacked ? f : g;
        const int x = x0 + lx, y = y0 + ly;
        if (x < W && y < H) {
            if (kPacked) {
                const int tp = x * H + y;
                if (o.tap16) { o.packed[tp] = s_a[lx][ly]; if (o.depthT) o.depthT[tp] = s_b[lx][ly].w; }
                else { o.packed[2 * tp] = s_a[lx][ly]; o.packed[2 * tp + 1] = s_b[lx][ly]; }
                if (o.maskT) o.maskT[tp] = s_mk[lx][ly];
            } else {
                const int p = y * W + x;
                o.index[p] = s_i[lx][ly]; o.vc[p] = s_a[lx][ly]; o.nr[p] = s_b[lx][ly];
                if (o.ct) o.ct[p] = s_c[lx][ly];
            }
        }
    }
}
// column-major keys -> the packed column-major map: keys and records in the same order, only the frame planes are transposed
__device__ __forceinline__ void index_resolve_packed_body(Surfels src, const PoseDev* __restrict__ pose, unsigned long long* __restrict__ keys, int W, int H,
                                                          ResolveOut o, int tile) {
    __shared__ float s_d[kResolveTile][kResolveTile + 1];
    __shared__ uint8_t s_mk[kResolveTile][kResolveTile + 1];
    const int tilesX = (W + kResolveTile - 1) / kResolveTile;
    const int x0 = (tile % tilesX) * kResolveTile, y0 = (tile / tilesX) * kResolveTile;
    const int f = threadIdx.x & (kResolveTile - 1), g = threadIdx.x / kResolveTile;
    const bool planes = o.maskT != nullptr;    // (the same in every workgroup of the launch)
    if (planes) {
        const int x = x0 + f, y = y0 + g;
        float d = 0.f;
        int mk = 0;
        if (x < W && y < H) { d = o.depthF[y * W + x]; mk = o.mask[y * W + x]; s_d[f][g] = d; s_mk[f][g] = (uint8_t)mk; }
        decay_stats_add(o, x < W && y < H, x, y, W, H, d, mk);
        __syncthreads();
    }
    const int x = x0 + g, y = y0 + f;
    if (x < W && y < H) {
        const int tp = x * H + y;
        const unsigned long long key = keys[tp];
        keys[tp] = kEmptyKey;
        const Tap16 t16{o.tapThreshold, (float)o.frame->tick};
        ResolvedTexel r = resolve_texel<true>(src, pose, key, false, o.frame->first, o.tap16 ? &t16 : nullptr);
        if (planes) r.p1.w = s_d[g][f];
        if (o.tap16) { o.packed[tp] = r.p0; if (planes) o.depthT[tp] = r.p1.w; }
        else { o.packed[2 * tp] = r.p0; o.packed[2 * tp + 1] = r.p1; }
        if (planes) o.maskT[tp] = s_mk[g][f];
    }
}
// (the model-by-model launches scatter column-major: the maps go through the transposing tile kernel, the packed map through k_index_resolve_packed;
// index_resolve_same_body and index_resolve_transposing_body<true> serve the object batch's row-major keys)
__global__ __launch_bounds__(256) void k_index_resolve_packed(Surfels src, const PoseDev* __restrict__ pose, unsigned long long* __restrict__ keys, int W, int H,
                                                              ResolveOut o) {
    index_resolve_packed_body(src, pose, keys, W, H, o, (int)blockIdx.x);
}
template <bool kPacked>
__global__ __launch_bounds__(256) void k_index_resolve_transposing(Surfels src, const PoseDev* __restrict__ pose, unsigned long long* __restrict__ keys, int W, int H,
                                                                   ResolveOut o) {
    index_resolve_transposing_body<kPacked>(src, pose, keys, W, H, o, (int)blockIdx.x);
}
int resolve_tiles(int W, int H) { return ((W + kResolveTile - 1) / kResolveTile) * ((H + kResolveTile - 1) / kResolveTile); }

void launch_index_resolve_maps(Surfels src, const PassFrame& f, const PassModel& m, bool want_ct, hipStream_t s) {
    hipLaunchKernelGGL(k_index_resolve_transposing<false>, dim3(resolve_tiles(f.W, f.H)), dim3(256), 0, s, src, m.pose, m.scr.keys, f.W, f.H,
                       resolve_out_maps(m, want_ct));
}
void launch_index_resolve_packed(Surfels src, const PassFrame& f, const PassModel& m, hipStream_t s, bool maskFree, int* decay_stats) {
    hipLaunchKernelGGL(k_index_resolve_packed, dim3(resolve_tiles(f.W, f.H)), dim3(256), 0, s, src, m.pose, m.scr.keys, f.W, f.H,
                       resolve_out_packed(f, m, maskFree, decay_stats));
}

// ------------------------------------------------------------------------------------------------
// data association (data.vert).  Threads walk candidates row-major (coalesced image reads); the candidate's
// column-major index c = xi * nyc + yi is only its slot / its priority in the first-writer-wins merge.
// ------------------------------------------------------------------------------------------------
// kLanes == 1: one thread per candidate walks the nine taps.  kLanes == 4: a quad of neighbouring lanes per candidate (16 candidates per wavefront);
// lanes 0, 1, 2 own the window columns da = -1, 0, +1 -- taps q = 3 lane .. 3 lane + 2 of the serial order -- and the three partial results are merged in
// lane order with the same strict <: the first arg-min over the gated taps in the order q = 0..8, which is what the serial loop computes.  Every
// lane of the quad computes the candidate's own values (same addresses, same operations); lane 0 stores.
template <int kLanes>
__device__ __forceinline__ void fuse_data_body(const FuseDataArgs& a) {
    static_assert(kLanes == 1 || kLanes == 4, "one lane or a quad per candidate");
    constexpr int kPerWave = 64 / kLanes, kTaps = kLanes == 1 ? 9 : 3;
    const int time = a.frame->tick;
    const int par = time & 1;
    const int W = a.W, H = a.H;
    const int nxc = (W - par + 1) / 2, nyc = (H - par + 1) / 2;
    const int ql = (int)threadIdx.x & (kLanes - 1);        // lane of the quad
    const int xi = blockIdx.x * kPerWave + ((threadIdx.x & 63) / kLanes);
    const int yi = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (xi >= nxc || yi >= nyc) return;                    // (whole quads leave together)
    const int c = xi * nyc + yi;
    const int px = 2 * xi + par, py = 2 * yi + par;
    const Intr k = a.k;
    uint8_t op = 0;
    const float x = (float)px + 0.5f, y = (float)py + 0.5f;
    // data.vert:139-141 window: pixel-centre offsets {-1,-0.5,0,+0.5} -> texels {x-1,x,x,x+1}; a revisited texel can
    // never replace itself (strict <), so the 3x3 distinct texels in first-visit order are equivalent.
    // All window loads are issued unconditionally and together: guarding vertConf / normRad behind the index and
    // z tests made every tap a chain of three dependent gathers (17.5 us for 77 k candidates).  With a quad per candidate they are issued before
    // the candidate's validity is known as well: their addresses depend on the pixel alone (lane 3 of a quad repeats lane 2's column and drops it).
    int cur9[kTaps]; float4 vc9[kTaps], nr9[kTaps];
    if (kLanes == 4 && a.maskID != 0) {
        // an OBJECT model's mask covers a small part of the image: a wavefront none of whose 16 candidates lies in it leaves before it requests anything
        // else (one lane per candidate left after the mask test and two depth texels; the 9-object scene S2: 1 047 frames/s without this, 1 085 on one lane)
        if (__ballot(a.mask[py * W + px] == a.maskID) == 0ull) {
            if (ql == 0) a.cand_op[c] = 0;
            return;
        }
    }
    if (kLanes == 4) {
#pragma unroll
        for (int j = 0; j < kTaps; ++j) {
            const int da = min(ql, 2) - 1, db = j - 1;
            const int tp = clampi(py + db, 0, H - 1) * W + clampi(px + da, 0, W - 1);
            cur9[j] = a.index[tp];
            vc9[j] = a.vc[tp];
            nr9[j] = a.nr[tp];
        }
    }
    const float3 vLocal = get_vertex(a.depthRaw, W, H, px, py, x, y, k);
    bool valid = a.mask[py * W + px] == a.maskID;
    valid = valid && !(texf(a.depthRaw, W, H, px - 1, py) == 0 || texf(a.depthRaw, W, H, px, py - 1) == 0 ||
                       texf(a.depthRaw, W, H, px + 1, py) == 0 || texf(a.depthRaw, W, H, px, py + 1) == 0);
    // Model::fuse's maxDepth uniform = min(depthCutoff, model.maxDepth, bb_max_z) (Model.cpp:480-501,527): an OBJECT model whose
    // bounding box exists (the GUI drew it after the previous frame) does not grow in depth beyond the box + 5 %.  The box's two corners are
    // taken to the camera frame with pose^-1 and only their z is used.
    float maxDepth = a.maxDepth;
    if (a.maskID != 0 && a.bboxLimit) {
        const FrameDev* f = a.frame;
        if (f->bbox[0] <= f->bbox[3] && f->bbox[1] <= f->bbox[4] && f->bbox[2] <= f->bbox[5]) {   // !lastBoundingBox.isEmpty()
            const float* Ri = a.pose->Ri; const float* ti = a.pose->ti;
            const float bbscale = 0.001f;
            const float zmin = ((Ri[6] * (bbscale * (float)f->bbox[0]) + Ri[7] * (bbscale * (float)f->bbox[1])) + Ri[8] * (bbscale * (float)f->bbox[2])) + ti[2];
            const float zmax = ((Ri[6] * (bbscale * (float)f->bbox[3]) + Ri[7] * (bbscale * (float)f->bbox[4])) + Ri[8] * (bbscale * (float)f->bbox[5])) + ti[2];
            const float lo = zmin < zmax ? zmin : zmax, hi = zmin < zmax ? zmax : zmin;
            maxDepth = fminf(maxDepth, hi + 0.05f * fabsf(hi - lo));
        }
    }
    valid = valid && (vLocal.z > 0 && vLocal.z <= maxDepth);
    float bestDist = 1000;
    int best = 0;
    bool merge = false;
    float3 vGlobal = f3(0, 0, 0), nGlobal = vGlobal, vF = vGlobal, nLocal = vGlobal;
    float weighting = 0.f, colour = 0.f;
    if (kLanes == 4) {   // the frame loads of a valid candidate, requested with the window's: image texels, clamped to the image
        vF = get_vertex(a.depthF, W, H, px, py, x, y, k);
        nLocal = get_normal_central(a.depthF, W, H, px, py, x, y, vF, k);
        const uint8_t* pc = a.rgb + (size_t)(py * W + px) * 3;
        colour = (float)((pc[0] << 16) + (pc[1] << 8) + pc[2]);
    }
    if (valid) {
        float R[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = a.pose->R[q];
        const float3 t = f3(a.pose->t[0], a.pose->t[1], a.pose->t[2]);
        vGlobal = mul33(R, vLocal) + t;
        if (kLanes == 1) {
            vF = get_vertex(a.depthF, W, H, px, py, x, y, k);
            nLocal = get_normal_central(a.depthF, W, H, px, py, x, y, vF, k);
            const uint8_t* pc = a.rgb + (size_t)(py * W + px) * 3;
            colour = (float)((pc[0] << 16) + (pc[1] << 8) + pc[2]);
        }
        nGlobal = mul33(R, nLocal);
        weighting = a.pose->fusionWeight * a.weightMultiplier;

        const float xl = (x - k.cx) * (1.0f / k.fx), yl = (y - k.cy) * (1.0f / k.fy);
        const float lambda = sqrtf(xl * xl + yl * yl + 1);
        const float3 ray = f3(xl, yl, 1);
        if (kLanes == 1) {
#pragma unroll
            for (int q = 0; q < kTaps; ++q) {
                const int da = q / 3 - 1, db = q % 3 - 1;
                const int tp = clampi(py + db, 0, H - 1) * W + clampi(px + da, 0, W - 1);
                cur9[q] = a.index[tp];
                vc9[q] = a.vc[tp];
                nr9[q] = a.nr[tp];
            }
        }
#pragma unroll
        for (int q = 0; q < kTaps; ++q) {
            const int current = cur9[q];
            if (current > 0 && ql < 3) {
                const float4 vc = vc9[q];
                const float zdiff = vc.z - vLocal.z;
                if (fabsf(zdiff * lambda) < 0.05f) {
                    const float dist = norm3(cross3(ray, f3(vc.x, vc.y, vc.z)));
                    const float4 nr = nr9[q];
                    const float3 nn = f3(nr.x, nr.y, nr.z);
                    const float ang = shader_acos(dot3(nn, nLocal) / (norm3(nn) * norm3(nLocal)));
                    if (dist < bestDist && (fabsf(nr.z) < 0.75f || fabsf(ang) < 0.5f)) {
                        merge = true; bestDist = dist; best = current;
                    }
                }
            }
        }
    }
    if (kLanes == 4) {
        // the quad's partial results, merged in lane order (every lane of the wavefront that has not left takes part in the exchange)
        const float myDist = bestDist;
        const int myBest = best;
        bestDist = 1000; best = 0; merge = false;
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const float d = __shfl(myDist, l, 4);
            const int b = __shfl(myBest, l, 4);
            if (d < bestDist) { merge = true; bestDist = d; best = b; }
        }
        if (ql != 0) return;
    }
    if (valid) {
        op = merge ? 1 : 2;
        a.cand_rec[c * 3 + 0] = make_float4(vGlobal.x, vGlobal.y, vGlobal.z, surfel_confidence(x, y, weighting, k));
        a.cand_rec[c * 3 + 1] = make_float4(colour, 0.f, (float)time, merge ? -1.f : -2.f);
        a.cand_rec[c * 3 + 2] = make_float4(nGlobal.x, nGlobal.y, nGlobal.z, surfel_radius(vF.z, nLocal.z, k));
        if (merge) {
            atomicMin(&a.upd_first[best], c);  // first writer (lowest column-major index) wins
            a.cand_best[c] = best;
        }
    }
    a.cand_op[c] = op;
}

template <int kLanes>
__global__ __launch_bounds__(256) void k_fuse_data(const FuseDataArgs a) { fuse_data_body<kLanes>(a); }

void launch_fuse_data(const FuseDataArgs& a, int lanes, hipStream_t s) {
    const int per_wave = lanes == 4 ? 16 : 64;
    dim3 grid(((a.W + 1) / 2 + per_wave - 1) / per_wave, ((a.H + 1) / 2 + 3) / 4);
    if (lanes == 4) hipLaunchKernelGGL(k_fuse_data<4>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_fuse_data<1>, grid, dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------------------
// surfel update (update.vert), IN PLACE.  The reference copies the whole buffer through transform feedback (Model.cpp:583-646) although
// only the surfels a candidate was merged into change -- at most P / 4 of them, of 26 M in a full map.  Here one thread per candidate
// updates "its" surfel where it stands (first writer wins: the candidate with the lowest column-major index owns the merge, decided by
// the atomicMin of the association pass) and re-arms the surfel's merge slot; no surfel reads another, so the values are the ones the
// copying form wrote (rounds 1-4: an N-sized pass of 100 B per surfel with the second index scatter riding on it).
// ------------------------------------------------------------------------------------------------
// update.vert:40-96 for one surfel and the candidate merged into it (records in registers)
__device__ __forceinline__ void surfel_merge(float4& pc, float4& ct, float4& nr, float4 mp, float4 mc, float4 mn, float time) {
    const float c_k = pc.w, a = mp.w;
    if (mn.w < (1.0f + 0.5f) * nr.w) {
        pc = make_float4(((c_k * pc.x) + (a * mp.x)) / (c_k + a), ((c_k * pc.y) + (a * mp.y)) / (c_k + a),
                         ((c_k * pc.z) + (a * mp.z)) / (c_k + a), c_k + a);
        const float3 oc = decode_color(ct.x), nc = decode_color(mc.x);
        ct = make_float4(encode_color(((c_k * oc.x) + (a * nc.x)) / (c_k + a), ((c_k * oc.y) + (a * nc.y)) / (c_k + a),
                                      ((c_k * oc.z) + (a * nc.z)) / (c_k + a)),
                         ct.y, ct.z, time);
        const float4 av = make_float4(((c_k * nr.x) + (a * mn.x)) / (c_k + a), ((c_k * nr.y) + (a * mn.y)) / (c_k + a),
                                      ((c_k * nr.z) + (a * mn.z)) / (c_k + a), ((c_k * nr.w) + (a * mn.w)) / (c_k + a));
        const float3 nn = normalize_gl(f3(av.x, av.y, av.z));
        nr = make_float4(nn.x, nn.y, nn.z, av.w);
    } else {
        pc.w = c_k + a;
        ct.w = time;
    }
}

__device__ __forceinline__ void fuse_update_body(Surfels s, const FrameDev* __restrict__ frame, int* __restrict__ upd_first,
                                                 const uint8_t* __restrict__ cand_op, const int* __restrict__ cand_best,
                                                 const float4* __restrict__ cand_rec, int W, int H) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cand_count(W, H, frame->tick)) return;
    if (cand_op[c] != 1) return;
    const int i = cand_best[c];
    if (i < 0 || i >= frame->phys) return;
    if (upd_first[i] != c) return;          // an earlier candidate owns this surfel's merge
    upd_first[i] = kNoUpdate;
    float4 pc = s.pc[i], ct = s.ct[i], nr = s.nr[i];
    surfel_merge(pc, ct, nr, cand_rec[c * 3 + 0], cand_rec[c * 3 + 1], cand_rec[c * 3 + 2], (float)frame->tick);
    s.pc[i] = pc; s.ct[i] = ct; s.nr[i] = nr;
}

// The same as a COPY src -> dst over the whole buffer with the second index scatter (predictIndices after fuse, MaskFusion.cpp:556) riding on
// the values just written (rounds 1-4): the form for SMALL maps, where one 12 us pass beats an in-place update + a scatter launch of its own
// (8 + 10 us at VGA) and the whole frame is a chain of such launches; on a 26.9 M-surfel map the copy is 100 B per surfel, 0.56 ms.
__device__ __forceinline__ void fuse_update_copy_body(Surfels src, Surfels dst, const FrameDev* __restrict__ frame, int* __restrict__ upd_first,
                                                      const float4* __restrict__ cand_rec, const IndexScatterArgs& ix) {
    const int n = frame->count;
    const float time = (float)frame->tick;
    float Ri[9];
    float3 ti = f3(0, 0, 0);
    if (ix.keys) {
#pragma unroll
        for (int q = 0; q < 9; ++q) Ri[q] = ix.pose->Ri[q];
        ti = f3(ix.pose->ti[0], ix.pose->ti[1], ix.pose->ti[2]);
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        float4 pc = src.pc[i], ct = src.ct[i], nr = src.nr[i];
        const int m = upd_first[i];
        if (m != kNoUpdate) {
            upd_first[i] = kNoUpdate;
            surfel_merge(pc, ct, nr, cand_rec[m * 3 + 0], cand_rec[m * 3 + 1], cand_rec[m * 3 + 2], time);
        }
        dst.pc[i] = pc; dst.ct[i] = ct; dst.nr[i] = nr;
        if (ix.keys) {   // k_index_scatter on the updated surfel (index_map.vert:40-60)
            const float3 h = mul33(Ri, f3(pc.x, pc.y, pc.z)) + ti;
            if (!(h.z > ix.maxDepth || h.z <= 0 || time - ct.w > (float)ix.timeDelta)) {
                const float u = ((ix.k.fx * h.x) / h.z) + ix.k.cx;
                const float v = ((ix.k.fy * h.y) / h.z) + ix.k.cy;
                if (u >= 0.f && u < (float)ix.W && v >= 0.f && v < (float)ix.H) {
                    const int p = ix.transposed ? (int)floorf(u) * ix.H + (int)floorf(v) : (int)floorf(v) * ix.W + (int)floorf(u);
                    zmin_key(&ix.keys[p], ((unsigned long long)__float_as_uint(h.z) << 32) | (unsigned)i);
                }
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_fuse_update_copy(Surfels src, Surfels dst, const FrameDev* __restrict__ frame, int* __restrict__ upd_first,
                                                          const float4* __restrict__ cand_rec, const IndexScatterArgs ix) {
    fuse_update_copy_body(src, dst, frame, upd_first, cand_rec, ix);
}
void launch_fuse_update_copy(Surfels src, Surfels dst, const PassFrame& f, const PassModel& m, bool scatter, hipStream_t s, int blocks) {
    hipLaunchKernelGGL(k_fuse_update_copy, dim3(blocks), dim3(256), 0, s, src, dst, m.frame, m.scr.upd_first, m.scr.cand_rec, index_scatter_args(f, m, scatter, 1));
}

__global__ __launch_bounds__(256) void k_fuse_update(Surfels s, const FrameDev* __restrict__ frame, int* __restrict__ upd_first,
                                                     const uint8_t* __restrict__ cand_op, const int* __restrict__ cand_best,
                                                     const float4* __restrict__ cand_rec, int W, int H) {
    fuse_update_body(s, frame, upd_first, cand_op, cand_best, cand_rec, W, H);
}

static inline int cand_blocks(int W, int H) { return (((W + 1) / 2) * ((H + 1) / 2) + 255) / 256; }

void launch_fuse_update(Surfels s, const PassFrame& f, const PassModel& m, hipStream_t st) {
    hipLaunchKernelGGL(k_fuse_update, dim3(cand_blocks(f.W, f.H)), dim3(256), 0, st, s, m.frame, m.scr.upd_first, m.scr.cand_op, m.scr.cand_best, m.scr.cand_rec,
                       f.W, f.H);
}

// ------------------------------------------------------------------------------------------------
// clean (copy_unstable.vert:53-157): pass 1 = per-element test + new confidence + per-workgroup counts;
// pass 2 = ordered copy.  Element i < count is an old surfel, element count + c is candidate c (only op == 2 live).
// ------------------------------------------------------------------------------------------------
// The window of copy_unstable.vert:85-86 along one axis, exactly as the shader text walks it: `for (i = c - 2s; i < c + 2s; i += s)` on an
// fp32 induction variable makes 4 steps in exact arithmetic and 4 OR 5 in fp32, depending on the rounding of the centre c (27 % of
// the x positions at 640 columns make 5); every step is a tap that COUNTS towards `count > 8` / `zCount > 4`.  A tap's texel is the
// floor of its coordinate snapped to 1/256 texel -- the rule under which the reference's own shader, compiled from its source
// (oracle/_ref/libmf_glsl.so), was executed and the CPU restatement's literal mode was checked against it bit for bit.  The taps
// are monotone and span two pixels: at most three distinct texels u[] with multiplicities m[] (an unused slot has m = 0).
__device__ __forceinline__ void window_slots_literal(float c, int size, int (&u)[3], int (&m)[3]) {
    const float fs = (float)size;
    const float step = (1.0f / (fs * 1.0f)) * 0.5f;     // indexXStep = stepX * 0.5 / scale, scale = FACTOR = 1
    const float half = (1.0f * step) * 2.0f;            // scale * indexXStep * windowMultiplier
    const float end = c + half;
    u[0] = u[1] = u[2] = 0; m[0] = m[1] = m[2] = 0;
    int s = -1, last = -1;                               // texels are >= 0 after the clamp
    float i = c - half;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        if (i < end) {
            const int t = clampi((int)floorf(rintf(i * fs * 256.0f) * (1.0f / 256.0f)), 0, size - 1);
            if (t != last) { s = min(s + 1, 2); u[s] = t; last = t; }
            m[s] += 1;
        }
        i += step;
    }
}

// one 16-byte tap into the two counting rules of copy_unstable.vert:92-106
__device__ __forceinline__ void clean_count_tap16(float4 t, int mult, float3 lp, float initTime, float radius, float lnz, int& count, int& zCount) {
    const float vz = fabsf(t.z);
    if (!isnan(t.z) && mult > 0) {
        const float dx = t.x - lp.x, dy = t.y - lp.y;
        if (t.w < initTime && vz > lp.z && vz - lp.z < 0.01f && sqrtf(dx * dx + dy * dy) < radius * 1.4f) count += mult;
        if (__float_as_int(t.z) < 0 && vz > lp.z && vz - lp.z > 0.01f && fabsf(lnz) > 0.85f) zCount += mult;
    }
}
// the window of 16-byte taps, kGroup (3: a column, 9: all) of them requested before the first is looked at
template <int kGroup>
__device__ __forceinline__ void clean_window_grouped(const CleanArgs& a, const int (&ux)[3], const int (&mx)[3], const int (&uy)[3], const int (&my)[3],
                                                     float3 lp, float initTime, float radius, float lnz, int& count, int& zCount) {
    const int W = a.W, H = a.H;
    // slot -> texel: an unused slot reads slot 0's texel again
    const int gx[3] = {ux[0], mx[1] > 0 ? ux[1] : ux[0], mx[2] > 0 ? ux[2] : ux[0]};
    const int gy[3] = {uy[0], my[1] > 0 ? uy[1] : uy[0], my[2] > 0 ? uy[2] : uy[0]};
    float4 t[3][3];
    if (kGroup == 9) {
#pragma unroll
        for (int q = 0; q < 9; ++q) t[q / 3][q % 3] = a.packed[a.transposed ? gx[q / 3] * H + gy[q % 3] : gy[q % 3] * W + gx[q / 3]];
    }
#pragma unroll
    for (int ia = 0; ia < 3; ++ia) {
        if (kGroup == 3) {
#pragma unroll
            for (int ib = 0; ib < 3; ++ib) t[ia][ib] = a.packed[a.transposed ? gx[ia] * H + gy[ib] : gy[ib] * W + gx[ia]];
        }
#pragma unroll
        for (int ib = 0; ib < 3; ++ib) clean_count_tap16(t[ia][ib], mx[ia] * my[ib], lp, initTime, radius, lnz, count, zCount);
    }
}
// decay: which factor the mask-disagreement rule applied to the confidence (0 none, 1: k, 2: 0.25 k) -- clean_decayed() re-applies it
// nr_lazy != nullptr: the surfel's normal / radius record is only fetched when the window is walked (it is not needed otherwise); `nr` is then ignored
// kTap16: a.packed holds the 16-byte tap {x, y, z', initTime} (tap16_encode: written by the resolve pass of the same enqueue, with this pass's
// threshold and tick) instead of the 32-byte record; a tap counts under the same conditions, bit for bit.
// kGroup (16-byte taps only): how many taps are requested before the first of them is looked at -- 1: each tap is loaded, tested, and only then
// the next one requested (nine dependent gathers); 3: the three taps of a window column ux[ia] together -- in the column-major packed map they
// are at most three neighbouring texels, mostly one cache line --; 9: the whole window.  count / zCount are integer sums of multiplicities: the
// same whatever the order.  An unused slot (multiplicity 0) is requested at the address of slot 0 and ignored: no branch stands between the loads.
// kMaskFree: the frame has no mask and the model is id 0 -- `maskValue != a.maskID` below is false for every surfel --: neither plane is read.
template <bool kTap16, int kGroup = 1, bool kMaskFree = false>
__device__ __forceinline__ bool clean_test(const CleanArgs& a, float4 pc, float4 ct, float4 nr, float time, const float* Ri,
                                           float3 ti, float& newconf, int& decay, const float4* nr_lazy = nullptr) {
    static_assert(kTap16 || (kGroup == 1 && !kMaskFree), "grouped taps and the mask-free form are forms of the 16-byte tap");
    static_assert(kGroup == 1 || kGroup == 3 || kGroup == 9, "a tap, a window column or the window");
    const int W = a.W, H = a.H;
    bool test = true;
    const float3 lp = mul33(Ri, f3(pc.x, pc.y, pc.z)) + ti;
    const float x = ((a.k.fx * lp.x) / lp.z) + a.k.cx;
    const float y = ((a.k.fy * lp.y) / lp.z) + a.k.cy;
    int count = 0, zCount = 0;
    if (time - ct.w < (float)a.timeDelta && lp.z > 0 && x > 0 && y > 0 && x < (float)W && y < (float)H) {
        if (nr_lazy) nr = *nr_lazy;
        const float3 ln = normalize_gl(mul33(Ri, f3(nr.x, nr.y, nr.z)));
        // copy_unstable.vert:86-87 samples a 4x4 window at offsets {-1,-0.5,0,+0.5} px; nearest fetches land on only 2 or
        // 3 distinct texels per axis, so the window is walked as <= 3x3 distinct texels weighted by their multiplicity
        // (identical counts, ~2.5x fewer gathers).
        int txs[4], tys[4];
        txs[0] = clampi((int)floorf(x - 1.0f), 0, W - 1); txs[1] = clampi((int)floorf(x - 0.5f), 0, W - 1);
        txs[2] = clampi((int)floorf(x), 0, W - 1);        txs[3] = clampi((int)floorf(x + 0.5f), 0, W - 1);
        tys[0] = clampi((int)floorf(y - 1.0f), 0, H - 1); tys[1] = clampi((int)floorf(y - 0.5f), 0, H - 1);
        tys[2] = clampi((int)floorf(y), 0, H - 1);        tys[3] = clampi((int)floorf(y + 0.5f), 0, H - 1);
        // the four fetches are monotone: t0 <= t1 <= t2 <= t3 and t1 is t0 or t2 -> three static slots {t0, t2, t3}
        int ux[3] = {txs[0], txs[2], txs[3]};
        int mx[3] = {1 + (txs[1] == txs[0]), 1 + (txs[1] != txs[0]) + (txs[3] == txs[2]), (txs[3] != txs[2]) ? 1 : 0};
        int uy[3] = {tys[0], tys[2], tys[3]};
        int my[3] = {1 + (tys[1] == tys[0]), 1 + (tys[1] != tys[0]) + (tys[3] == tys[2]), (tys[3] != tys[2]) ? 1 : 0};
        if (a.literal) {   // the shader text's own trip count (see window_slots_literal)
            window_slots_literal(x / (float)W, W, ux, mx);
            window_slots_literal(y / (float)H, H, uy, my);
        }
        constexpr bool kGrouped = kTap16 && kGroup > 1;
        if (kGrouped) clean_window_grouped<kGroup>(a, ux, mx, uy, my, lp, ct.z, nr.w, ln.z, count, zCount);
#pragma unroll
        for (int ia = 0; ia < (kGrouped ? 0 : 3); ++ia) {
#pragma unroll
            for (int ib = 0; ib < 3; ++ib) {
                const int tp = a.transposed ? ux[ia] * H + uy[ib] : uy[ib] * W + ux[ia];
                const int mult = mx[ia] * my[ib];
                if (mult <= 0) continue;   // (requesting these 32-byte records in groups before looking at any -- 6 + 3, all 9 -- was tried in rounds 2 and 5: slower at VGA, DESIGN.md "rejected")
                float4 v, c;
                int idx;
                bool upd = false;     // (16-byte tap) lastTime == tick
                if (kTap16) {
                    const float4 t = a.packed[tp];
                    idx = isnan(t.z) ? 0 : 1;
                    upd = __float_as_int(t.z) < 0;
                    v = make_float4(t.x, t.y, fabsf(t.z), 0.f);
                    c = make_float4(0.f, 0.f, t.w, 0.f);
                } else if (a.packed) {
                    v = a.packed[2 * tp];
                    const float4 r1 = a.packed[2 * tp + 1];
                    c = make_float4(0.f, 0.f, r1.x, r1.y);
                    idx = __float_as_int(r1.z);
                } else {
                    idx = a.index[tp];
                    v = a.vc[tp];
                    c = a.ct[tp];
                }
                if (idx > 0) {
                    const float dx = v.x - lp.x, dy = v.y - lp.y;
                    if (c.z < ct.z && (kTap16 || v.w > a.confThreshold) && v.z > lp.z && v.z - lp.z < 0.01f &&
                        sqrtf(dx * dx + dy * dy) < nr.w * 1.4f)
                        count += mult;
                    if ((kTap16 ? upd : c.w == time) && (kTap16 || v.w > a.confThreshold) && v.z > lp.z && v.z - lp.z > 0.01f && fabsf(ln.z) > 0.85f)
                        zCount += mult;
                }
            }
        }
    }
    if (count > 8 || zCount > 4) test = false;
    float w = ct.w;
    if (w == -2.f) w = time;
    if (w == -1.f || ((time - w) > 20 && pc.w < a.confThreshold)) test = false;
    if (w > 0 && time - w > (float)a.timeDelta) test = true;
    newconf = pc.w;
    decay = 0;
    if (kMaskFree) return test;
    // mask-disagreement decay, copy_unstable.vert:139-156 (nearest fetch, clamp to edge, NaN -> texel 0)
    const int fx_ = isnan(x) ? 0 : clampi((int)fminf(fmaxf(floorf(x), -1.f), (float)W), 0, W - 1);
    const int fy_ = isnan(y) ? 0 : clampi((int)fminf(fmaxf(floorf(y), -1.f), (float)H), 0, H - 1);
    // (with the packed map: the filtered depth rides in its spare word -- 16-byte tap: in the column-major plane depthT --, the mask in the
    // column-major plane beside it -- launch_index_resolve_packed)
    const float wDepth = kTap16 ? a.depthT[fx_ * H + fy_] : a.packed ? a.packed[2 * (fx_ * H + fy_) + 1].w : a.depthF[fy_ * W + fx_];
    const int maskValue = a.packed ? a.maskT[fx_ * H + fy_] : a.mask[fy_ * W + fx_];
    if (maskValue != a.maskID && maskValue < 255 && (wDepth > lp.z - 0.05f && wDepth < lp.z + 0.05f)) {
        const float kk = 0.5f + 0.5f * (1 - a.outlierCoeff / 10.0f);
        if (maskValue == 0) { newconf *= kk; decay = 1; }
        else if (a.maskID == 0) { newconf *= 0.25f * kk; decay = 2; }
        else { newconf *= kk; decay = 1; }
    }
    return test;
}
// the confidence clean_test returned for a record, from the record and the decay code alone (the same float operations)
__device__ __forceinline__ float clean_decayed(const CleanArgs& a, float conf, int decay) {
    const float kk = 0.5f + 0.5f * (1 - a.outlierCoeff / 10.0f);
    if (decay == 1) conf *= kk;
    else if (decay == 2) conf *= 0.25f * kk;
    return conf;
}

// ------------------------------------------------------------------------------------------------
// clean, two launches over a static partition: pass 1 = per-element test + new confidence + per-workgroup counts, pass 2 = ordered copy.
//   * SMALL maps (append == 0; rounds 1-4): every element -- the buffer's surfels and the frame's candidates -- src -> dst, a dense buffer;
//   * the tail of the IN-PLACE clean of big maps (append == 1, below): the candidates only; their survivors are appended behind the buffer's last
//     run, and their runs to its table.
// The surviving records, their order and the count are the same bits either way (tests/test_gpu_switches.py::test_clean_forms_agree).
// ------------------------------------------------------------------------------------------------
template <bool kTap16, int kGroup, bool kMaskFree>
__device__ __forceinline__ void clean_small_flags_body(const CleanArgs& a) {
    __shared__ int s_w[4];
    // elements below `count` are the buffer's slots, the others the candidates; `first`: the first element these passes handle
    const int count = a.append ? a.frame->phys : a.frame->count;
    const int first = a.append ? count : 0;
    const int ncand = cand_count(a.W, a.H, a.frame->tick);
    const int total = count + ncand;
    const float time = (float)a.frame->tick;
    float Ri[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Ri[q] = a.pose->Ri[q];
    const float3 ti = f3(a.pose->ti[0], a.pose->ti[1], a.pose->ti[2]);
    const int chunk = chunk_size(total - first);
    const int beg = first + blockIdx.x * chunk, end = min(total, beg + chunk);
    int kept = 0;
    for (int i = beg + threadIdx.x; i < end; i += 256) {
        bool keep = false;
        float nc = 0.f;
        int dk = 0;
        if (i < count) {
            keep = clean_test<kTap16, kGroup, kMaskFree>(a, a.src.pc[i], a.src.ct[i], make_float4(0, 0, 0, 0), time, Ri, ti, nc, dk, &a.src.nr[i]);
        } else {
            const int c = i - count;
            if (a.cand_op[c] == 2)
                keep = clean_test<kTap16, kGroup, kMaskFree>(a, a.cand_rec[c * 3 + 0], a.cand_rec[c * 3 + 1], make_float4(0, 0, 0, 0), time, Ri, ti, nc, dk, &a.cand_rec[c * 3 + 2]);
        }
        a.flags[i - first] = keep ? 1 : 0;
        a.newconf[i - first] = nc;
        kept += keep ? 1 : 0;
    }
    const int tot = block_sum_i(kept, s_w);
    if (threadIdx.x == 0) {
        a.block_counts[blockIdx.x] = tot;
        if (blockIdx.x == 0) {
            a.frame->countNext = count;  // snapshots for pass 2 (see FrameDev)
            a.frame->runsNext = a.frame->runs;
            if (a.maskID != 0 && !a.append)   // the compaction pass (next launch) accumulates this clean pass's box (append: on top of k_clean_runs')
                for (int q = 0; q < 6; ++q) a.frame->bbox_acc[q] = q < 3 ? kBBoxEmptyMin : kBBoxEmptyMax;
        }
    }
    if (a.append) {
        // the table entries pass 2 fills: new run j holds the output slots [count + j kRun, count + (j + 1) kRun)
        const int r0 = a.frame->runs, nnew = (ncand + kRun - 1) / kRun + 1;
        for (int j = blockIdx.x * 256 + threadIdx.x; j < nnew; j += gridDim.x * 256) {
            a.dst.box[kBoxStride * (r0 + j)] = make_int4(kBoxEmptyMin, kBoxEmptyMin, kBoxEmptyMin, kBoxEmptyMax);
            a.dst.box[kBoxStride * (r0 + j) + 1] = make_int4(kBoxEmptyMax, kBoxEmptyMax, kBoxEmptyMax, count + j * kRun);
            a.dst.box[kBoxStride * (r0 + j) + 2] = make_int4(0, kBoxEmptyMin, 0, 0);
        }
    }
}

template <bool kTap16, int kGroup, bool kMaskFree>
__global__ __launch_bounds__(256) void k_clean_small_flags(const CleanArgs a) { clean_small_flags_body<kTap16, kGroup, kMaskFree>(a); }

__device__ __forceinline__ void clean_small_compact_body(const CleanArgs& a) {
    __shared__ int s_w[4];
    __shared__ int s_bb[6];
    // Model::lastBoundingBox of an OBJECT model (Model.cpp:315-345 + draw_global_surface.vert:55-78: the box of the surfels the GUI draws --
    // confidence above the model's threshold -- in millimetres, truncated): accumulated here, where the frame's final records pass through
    // registers anyway; Model::fuse of the NEXT frame limits its depth with it (Model.cpp:480-501).  The background (id 0) never uses one.
    const bool bbox_on = a.maskID != 0;
    int bmin[3] = {kBBoxEmptyMin, kBBoxEmptyMin, kBBoxEmptyMin}, bmax[3] = {kBBoxEmptyMax, kBBoxEmptyMax, kBBoxEmptyMax};
    if (bbox_on && threadIdx.x < 6) s_bb[threadIdx.x] = threadIdx.x < 3 ? kBBoxEmptyMin : kBBoxEmptyMax;
    const int count = a.frame->countNext;
    const int first = a.append ? count : 0;
    const int total = count + cand_count(a.W, a.H, a.frame->tick);
    const int r0 = a.frame->runsNext;     // (append) the table entry of the first new run
    const float time = (float)a.frame->tick;
    const int chunk = chunk_size(total - first);
    const int beg = first + blockIdx.x * chunk, end = min(total, beg + chunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int i0 = beg; i0 < end; i0 += 256) {
        // every load of the slice is issued before anything depends on one of them (the keep flag, the record, the new
        // confidence, and -- first slice -- the workgroup's base offset): one memory latency per slice instead of three
        const int i = i0 + threadIdx.x;
        const bool in = i < end;
        uint8_t flag = 0;
        float nc = 0.f;
        float4 pc = make_float4(0, 0, 0, 0), ct = pc, nr = pc;
        if (in) {
            flag = a.flags[i - first];
            nc = a.newconf[i - first];
            if (i < count) { pc = a.src.pc[i]; ct = a.src.ct[i]; nr = a.src.nr[i]; }
            else { const int c = i - count; pc = a.cand_rec[c * 3 + 0]; ct = a.cand_rec[c * 3 + 1]; nr = a.cand_rec[c * 3 + 2]; }
        }
        if (i0 == beg) base = block_base(a.block_counts, s_w) + first;
        const bool keep = in && flag;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_w[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += s_w[w];
        const int tot = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        const int o = off + lane_rank(m);
        const bool written = keep && o < a.dst.cap;
        if (written) {
            pc.w = nc;
            if (ct.w == -2.f) ct.w = time;  // copy_unstable.vert:131
            a.dst.pc[o] = pc; a.dst.ct[o] = ct; a.dst.nr[o] = nr;
            if (bbox_on && pc.w > a.confThreshold) {   // draw_global_surface.vert:55 (unstable == 0), :69-78
                const int x = (int)(1000.f * pc.x), y = (int)(1000.f * pc.y), z = (int)(1000.f * pc.z);
                bmin[0] = min(bmin[0], x); bmin[1] = min(bmin[1], y); bmin[2] = min(bmin[2], z);
                bmax[0] = max(bmax[0], x); bmax[1] = max(bmax[1], y); bmax[2] = max(bmax[2], z);
            }
        }
        if (a.append) {
            // the appended surfels' runs: a wavefront's survivors are consecutive output slots, in at most two runs
            const int j = written ? (o - count) / kRun : 0x7FFFFFFF;
            const int j0 = wave_min_i(j);
            if (j0 != 0x7FFFFFFF) {
                for (int g = 0; g < 2; ++g) {
                    const bool mine = written && j == j0 + g;
                    const unsigned long long mm = __ballot(mine);
                    if (mm == 0ull) continue;
                    RunAcc acc;
                    acc.reset();
                    if (mine) acc.add(pc, ct.w);
                    int v[8] = {acc.lo[0], acc.lo[1], acc.lo[2], acc.tmax, acc.hi[0], acc.hi[1], acc.hi[2], acc.cmin};
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] = (q < 3 || q == 7) ? wave_min_i(v[q]) : wave_max_i(v[q]);
                    const bool unstamped = __ballot(acc.unstamped != 0) != 0ull;
                    if (lane == 0) {
                        int* e = reinterpret_cast<int*>(&a.dst.box[kBoxStride * (r0 + j0 + g)]);
                        atomicMin(&e[0], v[0]); atomicMin(&e[1], v[1]); atomicMin(&e[2], v[2]); atomicMax(&e[3], v[3]);
                        atomicMax(&e[4], v[4]); atomicMax(&e[5], v[5]); atomicMax(&e[6], v[6]);
                        atomicAdd(&e[8], __popcll(mm)); atomicMin(&e[9], v[7]);
                        if (unstamped) atomicMax(&e[10], 1);   // (a frame's new surfels are stamped with its tick: tick <= 0 only)
                    }
                }
            }
        }
        base += tot;
        __syncthreads();
    }
    if (bbox_on) {   // (the loop's barriers order the initialisation of s_bb before these; a workgroup without elements skips both)
        if (beg < end) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (bmin[q] != kBBoxEmptyMin) atomicMin(&s_bb[q], bmin[q]);
                if (bmax[q] != kBBoxEmptyMax) atomicMax(&s_bb[3 + q], bmax[q]);
            }
            __syncthreads();
            if (threadIdx.x < 3 && s_bb[threadIdx.x] != kBBoxEmptyMin) atomicMin(&a.frame->bbox_acc[threadIdx.x], s_bb[threadIdx.x]);
            else if (threadIdx.x >= 3 && threadIdx.x < 6 && s_bb[threadIdx.x] != kBBoxEmptyMax) atomicMax(&a.frame->bbox_acc[threadIdx.x], s_bb[threadIdx.x]);
        }
    }
    if (blockIdx.x != gridDim.x - 1) return;
    if (beg >= end) base = block_base(a.block_counts, s_w) + first;   // the last workgroup owns no elements: all threads take part
    if (threadIdx.x == 0) {
        const int end_slot = min(base, a.dst.cap);
        if (a.append) {
            // (nobody else reads these during the launch: the other workgroups work from the snapshots)
            const int n = a.frame->count + (end_slot - count);
            a.frame->count = n;
            a.frame->phys = end_slot;
            a.frame->runs = r0 + (end_slot - count + kRun - 1) / kRun;
            // the first live surfel: runs only lose surfels, so the first non-empty run moves forward only; if every old run is empty it is the first
            // appended surfel (an empty map has none: the value is never used)
            int fr = a.frame->first_run;
            while (fr < r0 && run_len(a.dst.box, fr) == 0) ++fr;
            a.frame->first_run = fr;
            a.frame->first = fr < r0 ? run_start(a.dst.box, fr) : count;
            if (a.host_count) *a.host_count = n;
            if (a.host_append) *a.host_append = append_mirror(a.seq, r0 + (end_slot - count + kRun - 1) / kRun, end_slot);
        } else {
            a.frame->count = a.frame->phys = end_slot;
            a.frame->runs = 0;   // a dense buffer; this form writes no run table
            a.frame->first = 0; a.frame->first_run = 0;
            if (a.host_count) *a.host_count = end_slot;
        }
    }
}

__global__ __launch_bounds__(256) void k_clean_small_compact(const CleanArgs a) { clean_small_compact_body(a); }

// ------------------------------------------------------------------------------------------------
// clean, IN PLACE (round 6): Model::clean of a big map as O(surfels its tests can change), not O(N).
// The reference streams the whole buffer through transform feedback every frame (Model.cpp:649-772: N x 48 B read, N' x 48 B written), and so did
// rounds 1-5 here (round 5: one launch with a decoupled look-back, 3.6 GB moved in 1.28 ms on the 26.9 M-surfel map of configs[4], >= 78 % of it
// copies of surfels no test of copy_unstable.vert:53-157 can touch).  What the pass can do to a surfel of the buffer:
//   (a) drop it by the window rules (:77-106)          -- only a surfel inside the image, in front of the camera, seen within timeDelta;
//   (b) drop it by the age rule (:118-125)             -- only an UNSTABLE surfel (confidence below the threshold) last seen within timeDelta, or
//       a surfel whose time stamp is <= 0 (-1: dropped whatever its confidence; unstable ones: the rescue of old surfels asks for a stamp > 0);
//   (c) lower its confidence, mask disagreement (:139-156) -- a surfel whose texel (clamped to the image border when it projects outside) carries a
//       foreign mask value and a filtered depth within 5 cm of its own.
// The buffer is kept as RUNS (Surfels::box): k_cull_clean lists the runs in which (a), (b) or (c) can apply at all -- from the run's box, its newest
// time stamp, its lowest confidence, and the frame's border / foreign-mask depth ranges (ResolveOut::decay_stats) -- and k_clean_runs visits only
// those: tests every surfel, and where a run loses surfels moves its survivors up INSIDE the run (their order is kept; the slots behind them stay
// unused).  The order of the surfels -- the reference's transform-feedback order, which decides z-test ties and which surfel is vertex 0 -- is the
// order of the runs; nothing ever moves between runs, so no workgroup waits for another (the round-5 look-back and its ticket order are gone).
// The frame's new surfels are appended behind the last run by the two-launch form above (append = 1).  When the slots behind the last run, or
// the table, run out, the host compacts the buffer (k_run_offsets + k_densify, mf_frame.inl) -- a copy of the live surfels, every few dozen frames.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cull_clean(Surfels s, const FrameDev* __restrict__ frame, const PoseDev* __restrict__ pose, int W, int H, Intr k,
                                                    int timeDelta, float confThreshold, int* __restrict__ decay_stats, int* __restrict__ list,
                                                    int* __restrict__ count, int* __restrict__ ctl) {
    const int runs = frame->runs;
    const float time = (float)frame->tick;
    const int r = blockIdx.x * 256 + threadIdx.x;
    // what the frame holds for rule (c): filtered depth of the border texels with a foreign mask, side by side; lowest filtered depth of ANY foreign texel
    int e_side[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) e_side[q] = decay_stats[q];
    const int e_amin = decay_stats[8];
    const bool has_any = e_amin != kBoxEmptyMin;
    bool visit = false;
    if (r < runs) {
        const int4 a = s.box[kBoxStride * r], b = s.box[kBoxStride * r + 1], c = s.box[kBoxStride * r + 2];
        if (c.x > 0) {
            const bool recent = !(time - box_dec(a.w) > (float)timeDelta);
            if (c.y != kBoxEmptyMin && box_dec(c.y) < confThreshold && recent) visit = true;              // (b)
            // (b) without an age limit: a stamp of -1 drops a surfel at any confidence, an unstable surfel stamped <= 0 is never rescued by
            // `lastTime > 0 && age > timeDelta` (copy_unstable.vert:134-136), and a stamp of -2 is replaced by the tick (:131)
            else if (c.z != 0) visit = true;
            else if (a.x <= b.x && a.y <= b.y && a.z <= b.z) {     // (a run of NaN positions only: every comparison of (a) and (c) fails)
                float zlo, zhi;
                int outside = 0;
                if (run_box_in_frustum(a, b, pose, W, H, k, INFINITY, zlo, zhi, &outside)) visit = true;  // (a), and (c) inside the image
                else if (zlo > 0.06f) {
                    // In front of the camera and outside the image: every surfel's texel is clamped to the border.  A box that lies beyond the LEFT
                    // edge as a whole puts all of them into the left column (any row), and so on: rule (c) needs a foreign texel THERE whose depth is
                    // within 5 cm of a surfel's -- one side that rules it out is enough.
                    visit = true;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if ((outside >> q) & 1) {
                            const bool has = e_side[2 * q] != kBoxEmptyMin;
                            if (!has || box_dec(e_side[2 * q + 1]) <= zlo - 0.06f || box_dec(e_side[2 * q]) >= zhi + 0.06f) visit = false;
                        }
                    if (outside == 0) visit = has_any;      // (outside by the near plane only: cannot happen with zlo > 0 -- kept conservative)
                } else if (zhi < -0.06f)     // behind the camera: any texel, but only a NEGATIVE filtered depth is within 5 cm (the filter writes none)
                    visit = has_any && box_dec(e_amin) < zhi + 0.06f;
                else visit = has_any;        // around the camera plane: any texel, depths around zero
            }
        }
    }
    run_list_append(visit, r, list, count, ctl);
    if (run_list_finish(count, ctl)) {       // every workgroup has read the statistics: armed for the next frame's resolve pass
        for (int q = 0; q < kDecayStats; ++q)
            __hip_atomic_store(&decay_stats[q], (q == 8 || (q & 1) == 0) ? kBoxEmptyMin : kBoxEmptyMax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__global__ void k_arm_decay_stats(int* st) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        for (int q = 0; q < kDecayStats; ++q) st[q] = (q == 8 || (q & 1) == 0) ? kBoxEmptyMin : kBoxEmptyMax;
}
void launch_arm_decay_stats(int* stats, hipStream_t st) { hipLaunchKernelGGL(k_arm_decay_stats, dim3(1), dim3(64), 0, st, stats); }
void launch_cull_clean(Surfels s, const FrameDev* frame, const PoseDev* pose, int W, int H, Intr k, int timeDelta, float confThreshold, int* decay_stats,
                       int* list, int* count, int* ctl, int max_runs, hipStream_t st) {
    hipLaunchKernelGGL(k_cull_clean, dim3((max_runs + 255) / 256), dim3(256), 0, st, s, frame, pose, W, H, k, timeDelta, confThreshold, decay_stats, list,
                       count, ctl);
}

// One run per workgroup and round (its <= kRun slots: two per thread); the runs are dealt round-robin over the grid (the listed runs come in no
// particular order, expensive -- in view -- and cheap ones mixed).
template <bool kTap16, int kGroup, bool kMaskFree>
__device__ __forceinline__ void clean_runs_body(const CleanArgs& a) {
    __shared__ int s_cnt[2][4];
    __shared__ int s_red[4][kRunRed];
    __shared__ int s_bb[6];
    static_assert(kRun == 512, "two slots per thread");
    // Model::lastBoundingBox of an OBJECT model: see clean_small_compact_body (here: the box of the buffer's own survivors; the append pass adds
    // the new surfels').  An object model's launch therefore visits EVERY run.
    const bool bbox_on = a.maskID != 0;
    int bmin[3] = {kBBoxEmptyMin, kBBoxEmptyMin, kBBoxEmptyMin}, bmax[3] = {kBBoxEmptyMax, kBBoxEmptyMax, kBBoxEmptyMax};
    if (bbox_on && threadIdx.x < 6) s_bb[threadIdx.x] = threadIdx.x < 3 ? kBBoxEmptyMin : kBBoxEmptyMax;
    const int nlist = a.run_list ? *a.run_count : a.frame->runs;     // (frame->runs / count change behind this launch only)
    const float time = (float)a.frame->tick;
    float Ri[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Ri[q] = a.pose->Ri[q];
    const float3 ti = f3(a.pose->ti[0], a.pose->ti[1], a.pose->ti[2]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int wg_died = 0;          // surfels this workgroup dropped (thread 0's copy is the one that counts)
    for (int v = blockIdx.x; v < nlist; v += gridDim.x) {
        const int r = a.run_list ? a.run_list[v] : v;
        const int start = run_start(a.src.box, r), len = run_len(a.src.box, r);
        // The test needs HALF of a record -- position + confidence, the two time stamps: 24 of its 48 bytes; the normal / radius record only for a
        // surfel in view (clean_test fetches it there), the rest only for a survivor that moves.  Slots threadIdx.x and 256 + threadIdx.x of the run.
        const int off0 = (int)threadIdx.x, off1 = 256 + (int)threadIdx.x;
        const bool live0 = off0 < len, live1 = off1 < len;
        float4 pc0 = make_float4(0, 0, 0, 0), pc1 = pc0;
        float2 tm0 = make_float2(0, 0), tm1 = tm0;
        if (live0) { pc0 = a.src.pc[start + off0]; tm0 = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(&a.src.ct[start + off0]) + 2); }
        if (live1) { pc1 = a.src.pc[start + off1]; tm1 = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(&a.src.ct[start + off1]) + 2); }
        // (Requesting every load of an element's test at once -- normal / radius, the nine window records, the mask texel: 135 registers -- changed
        // nothing on the configs[4] maps, 0.43 ms either way: the pass is bound by the instructions of the test, ~2 000 per surfel in view.)
        float nc0 = 0.f, nc1 = 0.f;
        int dk = 0;
        const bool keep0 = live0 && clean_test<kTap16, kGroup, kMaskFree>(a, pc0, make_float4(0.f, 0.f, tm0.x, tm0.y), make_float4(0, 0, 0, 0), time, Ri, ti, nc0, dk, &a.src.nr[start + off0]);
        const bool keep1 = live1 && clean_test<kTap16, kGroup, kMaskFree>(a, pc1, make_float4(0.f, 0.f, tm1.x, tm1.y), make_float4(0, 0, 0, 0), time, Ri, ti, nc1, dk, &a.src.nr[start + off1]);
        RunAcc acc;
        acc.reset();
        // copy_unstable.vert:131: a surfel stamped -2 ("seen in this frame") leaves the pass stamped with the tick -- only an uploaded map holds one
        const bool st0 = keep0 && tm0.y == -2.f, st1 = keep1 && tm1.y == -2.f;
        if (keep0) acc.add(make_float4(pc0.x, pc0.y, pc0.z, nc0), st0 ? time : tm0.y);
        if (keep1) acc.add(make_float4(pc1.x, pc1.y, pc1.z, nc1), st1 ? time : tm1.y);
        const unsigned long long m0 = __ballot(keep0), m1 = __ballot(keep1);
        if (lane == 0) { s_cnt[0][wave] = __popcll(m0); s_cnt[1][wave] = __popcll(m1); }
        int o0 = lane_rank(m0), o1 = lane_rank(m1);
        run_box_reduce(acc, s_red);
        __syncthreads();
        const int c0 = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
        const int kept = c0 + s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
        for (int w = 0; w < wave; ++w) { o0 += s_cnt[0][w]; o1 += s_cnt[1][w]; }
        o1 += c0;
        const bool conf0 = keep0 && __float_as_int(nc0) != __float_as_int(pc0.w), conf1 = keep1 && __float_as_int(nc1) != __float_as_int(pc1.w);
        if (kept != len) {
            // the run lost surfels: its survivors behind the first hole move up, whole records, in order
            const bool mv0 = keep0 && o0 != off0, mv1 = keep1 && o1 != off1;
            float4 c40 = make_float4(0, 0, 0, 0), n40 = c40, c41 = c40, n41 = c40;
            if (mv0) { c40 = a.src.ct[start + off0]; n40 = a.src.nr[start + off0]; }
            if (mv1) { c41 = a.src.ct[start + off1]; n41 = a.src.nr[start + off1]; }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every record that moves is in registers before any slot of the run is rewritten
            __syncthreads();
            if (st0) c40.w = time;
            if (st1) c41.w = time;
            if (mv0) { a.src.pc[start + o0] = make_float4(pc0.x, pc0.y, pc0.z, nc0); a.src.ct[start + o0] = c40; a.src.nr[start + o0] = n40; }
            else {
                if (conf0) reinterpret_cast<float*>(&a.src.pc[start + off0])[3] = nc0;
                if (st0) reinterpret_cast<float*>(&a.src.ct[start + off0])[3] = time;
            }
            if (mv1) { a.src.pc[start + o1] = make_float4(pc1.x, pc1.y, pc1.z, nc1); a.src.ct[start + o1] = c41; a.src.nr[start + o1] = n41; }
            else {
                if (conf1) reinterpret_cast<float*>(&a.src.pc[start + off1])[3] = nc1;
                if (st1) reinterpret_cast<float*>(&a.src.ct[start + off1])[3] = time;
            }
        } else {     // nobody moves: only a decayed confidence (and a -2 stamp's replacement) is written
            if (conf0) reinterpret_cast<float*>(&a.src.pc[start + off0])[3] = nc0;
            if (conf1) reinterpret_cast<float*>(&a.src.pc[start + off1])[3] = nc1;
            if (st0) reinterpret_cast<float*>(&a.src.ct[start + off0])[3] = time;
            if (st1) reinterpret_cast<float*>(&a.src.ct[start + off1])[3] = time;
        }
        if (threadIdx.x == 0) {
            run_box_store(a.src.box, r, start, kept, s_red);
            wg_died += len - kept;
        }
        if (bbox_on) {   // draw_global_surface.vert:55 (unstable == 0), :69-78
            if (keep0 && nc0 > a.confThreshold) {
                const int x = (int)(1000.f * pc0.x), y = (int)(1000.f * pc0.y), z = (int)(1000.f * pc0.z);
                bmin[0] = min(bmin[0], x); bmin[1] = min(bmin[1], y); bmin[2] = min(bmin[2], z);
                bmax[0] = max(bmax[0], x); bmax[1] = max(bmax[1], y); bmax[2] = max(bmax[2], z);
            }
            if (keep1 && nc1 > a.confThreshold) {
                const int x = (int)(1000.f * pc1.x), y = (int)(1000.f * pc1.y), z = (int)(1000.f * pc1.z);
                bmin[0] = min(bmin[0], x); bmin[1] = min(bmin[1], y); bmin[2] = min(bmin[2], z);
                bmax[0] = max(bmax[0], x); bmax[1] = max(bmax[1], y); bmax[2] = max(bmax[2], z);
            }
        }
        __syncthreads();   // s_cnt / s_red are rewritten by the next round
    }
    if (bbox_on) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (bmin[q] != kBBoxEmptyMin) atomicMin(&s_bb[q], bmin[q]);
            if (bmax[q] != kBBoxEmptyMax) atomicMax(&s_bb[3 + q], bmax[q]);
        }
        __syncthreads();
        // (RETURNING atomics whose results are waited for: the "finished" ticket below must not overtake them -- a fire-and-forget atomic is not
        // ordered against a later one to another address)
        int seen = 0;
        if (threadIdx.x < 3 && s_bb[threadIdx.x] != kBBoxEmptyMin) seen = atomicMin(&a.frame->bbox_tmp[threadIdx.x], s_bb[threadIdx.x]);
        else if (threadIdx.x >= 3 && threadIdx.x < 6 && s_bb[threadIdx.x] != kBBoxEmptyMax) seen = atomicMax(&a.frame->bbox_tmp[threadIdx.x], s_bb[threadIdx.x]);
        if (threadIdx.x < 6) s_bb[threadIdx.x] = seen;      // (consumes the returned values)
    }
    // The last workgroup to FINISH installs the launch's results: one 64-bit atomic per workgroup carries both its "finished" ticket and the number
    // of surfels it dropped -- the value travels IN the atomic, so the workgroup that draws the last ticket holds the launch's total without any
    // ordering between workgroups.
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* done64 = reinterpret_cast<unsigned long long*>(a.ctl + 2);
        const unsigned long long old = atomicAdd(done64, (1ull << 32) | (unsigned long long)(unsigned)wg_died);
        if ((unsigned)(old >> 32) == gridDim.x - 1u) {
            const int n = a.frame->count - ((int)(unsigned)(old & 0xFFFFFFFFull) + wg_died);
            a.frame->count = n;
            if (a.host_count) *a.host_count = n;
            if (bbox_on) {   // the box of a frame is the box of its LAST clean pass (the reference's render pass sees the final buffer)
                for (int q = 0; q < 6; ++q) {
                    a.frame->bbox_acc[q] = __hip_atomic_load(&a.frame->bbox_tmp[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&a.frame->bbox_tmp[q], q < 3 ? kBBoxEmptyMin : kBBoxEmptyMax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            __hip_atomic_store(done64, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <bool kTap16, int kGroup, bool kMaskFree>
__global__ __launch_bounds__(256) void k_clean_runs(const CleanArgs a) { clean_runs_body<kTap16, kGroup, kMaskFree>(a); }

// workgroups of a k_clean_runs launch for a buffer of ~`elements` surfels: the runs are dealt round-robin, any grid covers any table
int clean_runs_grid(long elements) {
    const long runs = (elements + kRun - 1) / kRun;
    return (int)(runs < 64 ? 64 : (runs > kCleanGridMax ? kCleanGridMax : runs));
}

// ------------------------------------------------------------------------------------------------
// compaction of a sparse buffer: src's runs -> dst, dense (slots [0, count), no table).  Host-driven (mf_frame.inl: densify), when the slots
// behind the last run or the table entries run out, before a download, before a model's passes return to the small-map forms.
// ------------------------------------------------------------------------------------------------
// offs[r] = live surfels of the runs before run r, offs[runs] = all of them; *total (optional) = the buffer's live surfels, also of a dense buffer
// without a table (runs == 0: offs[0] = 0, *total = count).  One workgroup.
__global__ __launch_bounds__(1024) void k_run_offsets(Surfels s, const FrameDev* __restrict__ frame, int* __restrict__ offs, int* __restrict__ total) {
    __shared__ int s_w[16];
    const int runs = frame->runs;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < runs; base += 1024) {
        const int r = base + (int)threadIdx.x;
        const int v = r < runs ? run_len(s.box, r) : 0;
        const int x = wave_scan(v, lane);
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        int before = 0, sum = 0;
        for (int w = 0; w < 16; ++w) { if (w < wave) before += s_w[w]; sum += s_w[w]; }
        if (r < runs) offs[r] = carry + before + x - v;
        carry += sum;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        offs[runs] = carry;
        if (total) *total = runs > 0 ? carry : frame->count;
    }
}
void launch_run_offsets(Surfels s, const FrameDev* frame, int* offs, int* total, hipStream_t st) {
    hipLaunchKernelGGL(k_run_offsets, dim3(1), dim3(1024), 0, st, s, frame, offs, total);
}
__global__ __launch_bounds__(256) void k_densify(Surfels src, Surfels dst, const FrameDev* __restrict__ frame, const int* __restrict__ offs) {
    for_each_live_ordered(src, frame, offs, dst.cap, [&](int from, int to) {
        dst.pc[to] = src.pc[from]; dst.ct[to] = src.ct[from]; dst.nr[to] = src.nr[from];
    });
}
__global__ void k_densify_finish(FrameDev* __restrict__ frame, const int* __restrict__ offs, int cap, int* __restrict__ host_count) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int n = min(offs[frame->runs], cap);
    frame->count = frame->phys = n;
    frame->runs = 0; frame->first = 0; frame->first_run = 0;
    if (host_count) *host_count = n;
}
void launch_densify(Surfels src, Surfels dst, FrameDev* frame, int* offs, int* host_count, hipStream_t st) {
    launch_run_offsets(src, frame, offs, nullptr, st);
    hipLaunchKernelGGL(k_densify, dim3(2048), dim3(256), 0, st, src, dst, frame, offs);
    hipLaunchKernelGGL(k_densify_finish, dim3(1), dim3(64), 0, st, frame, offs, dst.cap, host_count);
}

// ------------------------------------------------------------------------------------------------
// splat prediction: scatter (sprite_scatter_body, mf_sprite_device.h: per-surfel sprite loop, ray-disc test, 64-bit atomicMin with the
// surfel's index as the key's low word -- the lower index wins ties) + resolve
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_splat_scatter(const SpriteView v, unsigned long long* __restrict__ keys) { sprite_scatter_body<1, true>(v, 0u, keys, false); }

void launch_splat_scatter(const SpriteView& v, unsigned long long* keys, hipStream_t s, int blocks) {
    hipLaunchKernelGGL(k_splat_scatter, dim3(blocks), dim3(256), 0, s, v, keys);
}

__device__ __forceinline__ void splat_resolve_body(const SpriteView& v, unsigned long long* __restrict__ keys, const PredOut& o) {
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= v.W || py >= v.H) return;
    const int W = v.W, H = v.H;
    const Intr k = v.k;
    const int p = py * W + px;
    const unsigned long long key = keys[p];
    keys[p] = kEmptyKey;
    if (key == kEmptyKey) {
        o.predV[p] = o.predN[p] = make_float4(0, 0, 0, 0);
        o.predImage[p] = make_uchar4(0, 0, 0, 0);
        o.predTime[p] = 0;
        // intensity images for the photometric term of the NEXT tracking step (imageBGRToIntensity of the RGB projection,
        // and of the fill-in image: fill_rgb.frag takes the raw frame where the projection is empty)
        if (o.predGray) o.predGray[p] = 0;
        if (o.fillGray && o.rgb) o.fillGray[p] = intensity_of((float)o.rgb[p * 3], (float)o.rgb[p * 3 + 1], (float)o.rgb[p * 3 + 2]);
        return;
    }
    const int i = (int)(unsigned)(key & 0xFFFFFFFFull);
    const float z = __uint_as_float((unsigned)(key >> 32));
    const float4 pc = v.src.pc[i], c4 = v.src.ct[i], n4 = v.src.nr[i];
    const float3 n = normalize_gl(mul33(v.pose->Ri, f3(n4.x, n4.y, n4.z)));
    const float fcx = (float)px + 0.5f, fcy = (float)py + 0.5f;
    o.predV[p] = make_float4((fcx - k.cx) * z * (1.f / k.fx), (fcy - k.cy) * z * (1.f / k.fy), z, pc.w);  // combo_splat.frag:56
    o.predN[p] = make_float4(n.x, n.y, n.z, n4.w);
    const int ci = (int)c4.x;
    const uchar4 col = make_uchar4((ci >> 16) & 0xFF, (ci >> 8) & 0xFF, ci & 0xFF, 255);
    o.predImage[p] = col;
    o.predTime[p] = (uint16_t)(unsigned)c4.z;
    if (o.predGray || o.fillGray) {
        const uint8_t gv = intensity_of((float)col.x, (float)col.y, (float)col.z);
        if (o.predGray) o.predGray[p] = gv;
        if (o.fillGray) {
            // fill_rgb.frag:31-34: the raw frame where the projection is empty -- or everywhere with `passthrough` (frameToFrameRGB, Model.cpp:981)
            const bool empty = (col.x == 0 && col.y == 0 && col.z == 0) || o.fillPassthrough != 0;
            o.fillGray[p] = (empty && o.rgb) ? intensity_of((float)o.rgb[p * 3], (float)o.rgb[p * 3 + 1], (float)o.rgb[p * 3 + 2]) : gv;
        }
    }
    // MaskFusion::requiresFillIn (MaskFusion.cpp:630-648): nearest sample of the 20x down-sampled colour prediction
    if ((px % 20) == 10 && (py % 20) == 10 && px / 20 < W / 20 && py / 20 < H / 20 && col.x > 0 && col.y > 0 && col.z > 0)
        atomicAdd(&v.frame->cover, 1);
}

__global__ __launch_bounds__(256) void k_splat_resolve(const SpriteView v, unsigned long long* __restrict__ keys, const PredOut o) { splat_resolve_body(v, keys, o); }

void launch_splat_resolve(const SpriteView& v, unsigned long long* keys, const PredOut& out, hipStream_t s) {
    dim3 grid((v.W + 63) / 64, (v.H + 3) / 4);
    hipLaunchKernelGGL(k_splat_resolve, grid, dim3(256), 0, s, v, keys, out);
}

// ------------------------------------------------------------------------------------------------
// end of frame: tick++ and the fill-in decision for the next tracking step
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void frame_advance_body(FrameDev* frame, int W, int H, FrameDev* host_mirror, const PoseDev* pose, const PoseDev* bg_pose,
                                                   float* log_slot) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (log_slot) pose_log_entry(pose, bg_pose, log_slot);
    const int rw = W / 20, rh = H / 20;
    frame->pad[0] = frame->useFillIn;  // decision the tracking step of THIS frame ran with (mf_get_last_fillin)
    frame->useFillIn = ((float)frame->cover / (float)(rw * rh) < 0.75f) ? 1 : 0;
    frame->cover = 0;
    frame->tick += 1;
    MF_FRAME_BBOX_ADVANCE(frame);
    if (host_mirror) *host_mirror = *frame;
}
__global__ void k_frame_advance(FrameDev* frame, int W, int H, FrameDev* host_mirror, const PoseDev* pose, const PoseDev* bg_pose,
                                float* log_slot) {
    frame_advance_body(frame, W, H, host_mirror, pose, bg_pose, log_slot);
}
void launch_frame_advance(FrameDev* frame, int W, int H, FrameDev* host_mirror, const PoseDev* pose, const PoseDev* bg_pose,
                          float* log_slot, hipStream_t s) {
    hipLaunchKernelGGL(k_frame_advance, dim3(1), dim3(64), 0, s, frame, W, H, host_mirror, pose, bg_pose, log_slot);
}

// the pose-log entry alone (MaskFusion.cpp:580-596): what the frame advance writes, as a launch of its own behind a captured frame
__global__ void k_pose_log(const PoseDev* __restrict__ pose, const PoseDev* __restrict__ bg_pose, float* __restrict__ slot) {
    if (threadIdx.x == 0 && blockIdx.x == 0) pose_log_entry(pose, bg_pose, slot);
}
void launch_pose_log(const PoseDev* pose, const PoseDev* bg_pose, float* slot, hipStream_t s) {
    hipLaunchKernelGGL(k_pose_log, dim3(1), dim3(64), 0, s, pose, bg_pose, slot);
}

// Workgroups of the two ordered-compaction launches for `elements` elements (the host's last known count: any grid is correct).  A VGA map
// (0.75 M elements) is fastest on 2 048 (303.6 against 309-313 us per frame on 1 024 and 305.0 on 4 096); from ~1.5 M elements on, 1 024 workgroups
// with longer slices win: 1280 x 960 on its natural map 847 -> 835 us, the four 3.7 M-element object maps of configs[4] 4.16 -> 4.07-4.12 ms
// (profiles/r06zo_ab.txt, r06zp_ab.txt).
// The instance of a clean kernel K<kTap16, kGroup, kMaskFree> for a pass's tap form: the 32-byte record or the separate images, or 16-byte taps by
// group ("cleanTapGroup": 1, 3 or 9 -- mf_set_param refuses everything else), without the mask planes where the pass drops them.  kMayDrop is a
// compile-time constant: the object batch passes false and no mask-free instance of its kernels exists.
#define MF_LAUNCH_CLEAN_GROUP(K, kMaskFree, group, grid, s, arg)                                                            \
    do {                                                                                                                    \
        if ((group) == 3) hipLaunchKernelGGL((K<true, 3, kMaskFree>), grid, dim3(256), 0, s, arg);                          \
        else if ((group) == 9) hipLaunchKernelGGL((K<true, 9, kMaskFree>), grid, dim3(256), 0, s, arg);                     \
        else hipLaunchKernelGGL((K<true, 1, kMaskFree>), grid, dim3(256), 0, s, arg);                                       \
    } while (0)
#define MF_LAUNCH_CLEAN(K, kMayDrop, tap16, group, maskFree, grid, s, arg)                                                  \
    do {                                                                                                                    \
        if (!(tap16)) hipLaunchKernelGGL((K<false, 1, false>), grid, dim3(256), 0, s, arg);                                 \
        else if (kMayDrop && (maskFree)) MF_LAUNCH_CLEAN_GROUP(K, kMayDrop, group, grid, s, arg);                           \
        else MF_LAUNCH_CLEAN_GROUP(K, false, group, grid, s, arg);                                                          \
    } while (0)
int compact_blocks_for(long elements) { return elements >= 1500000L ? kCompactBlocks / 2 : kCompactBlocks; }
void launch_clean_small(const CleanArgs& a, hipStream_t s, int blocks) {
    MF_LAUNCH_CLEAN(k_clean_small_flags, true, a.tap16, a.tapGroup, a.maskFree, dim3(blocks), s, a);
    hipLaunchKernelGGL(k_clean_small_compact, dim3(blocks), dim3(256), 0, s, a);
}
void launch_clean_runs(CleanArgs a, const VisList* runs, int blocks, hipStream_t s) {
    a.run_list = runs ? runs->list : nullptr; a.run_count = runs ? runs->count : nullptr;
    MF_LAUNCH_CLEAN(k_clean_runs, true, a.tap16, a.tapGroup, a.maskFree, dim3(blocks), s, a);
}
void launch_clean_append(CleanArgs a, hipStream_t s) {
    a.append = 1;
    // (the candidates are <= P / 4 elements: a grid of one 256-element slice per workgroup, at most kCompactBlocks of them)
    MF_LAUNCH_CLEAN(k_clean_small_flags, true, a.tap16, a.tapGroup, a.maskFree, dim3(kCompactBlocks), s, a);
    hipLaunchKernelGGL(k_clean_small_compact, dim3(kCompactBlocks), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------------------------
// The surfel passes of every OBJECT model of a frame, one launch per pass (grid.z = model; mf_internal.h: ObjBatch = the frame's PassFrame + a
// device array of PassModel + the launch's form).  Same bodies as the model-by-model launches of enqueue_fuse_clean / enqueue_predict
// (mf_frame.inl), whose kernel arguments come from the same builders (mf_internal.h: resolve_out_maps / _packed, fuse_data_args,
// index_scatter_args, clean_args) over the same two structs -- the results are bit-identical
// (tests/test_gpu_multimodel.py::test_object_model_launch_switches_change_nothing, ::test_batched_object_passes_agree_in_every_form) -- but a
// frame with M objects costs 9 launches instead of 9 M.  Core/MaskFusion.cpp:539-569 runs the models one after the other; nothing couples them.
// (The object models' keys are row-major in both index passes: index_scatter_one.)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_obj_index_scatter(const ObjBatch b) {
    const PassModel& m = b.m[blockIdx.z];
    index_scatter_body(m.a, m.frame, m.pose, b.W, b.H, b.k, b.maxDepthProcessed, b.timeDelta, m.scr.keys, 0, nullptr, nullptr, true);
}
__global__ __launch_bounds__(256) void k_obj_index_resolve(const ObjBatch b) {
    const PassModel& m = b.m[blockIdx.z];
    index_resolve_same_body<false>(m.a, m.pose, m.scr.keys, b.W * b.H, resolve_out_maps(m, false));
}
__global__ __launch_bounds__(256) void k_obj_index_resolve_packed(const ObjBatch b) {   // the pass that feeds clean(): grid.x = 16 x 16-pixel tiles
    const PassModel& m = b.m[blockIdx.z];
    index_resolve_transposing_body<true>(b.updateCopy ? m.b : m.a, m.pose, m.scr.keys, b.W, b.H, resolve_out_packed(b, m), (int)blockIdx.x);
}
template <int kLanes>
__global__ __launch_bounds__(256) void k_obj_fuse_data(const ObjBatch b) { fuse_data_body<kLanes>(fuse_data_args(b, b.m[blockIdx.z])); }
__global__ __launch_bounds__(256) void k_obj_fuse_update(const ObjBatch b) {
    const PassModel& m = b.m[blockIdx.z];
    fuse_update_body(m.a, m.frame, m.scr.upd_first, m.scr.cand_op, m.scr.cand_best, m.scr.cand_rec, b.W, b.H);
}
__global__ __launch_bounds__(256) void k_obj_fuse_update_copy(const ObjBatch b) {   // small models: a -> b with the second index scatter riding
    const PassModel& m = b.m[blockIdx.z];
    fuse_update_copy_body(m.a, m.b, m.frame, m.scr.upd_first, m.scr.cand_rec, index_scatter_args(b, m, true, 0));
}
// copy-update: fuse copied a -> b, clean goes b -> a (the live buffer stays); in-place update + two-launch clean: clean goes a -> b;
// in-place clean (cleanSmall == 0): everything happens in a, the two-launch form appends
__device__ __forceinline__ CleanArgs obj_clean_args(const ObjBatch& b, const PassModel& m, int append) {
    return clean_args(b, m, b.updateCopy ? m.b : m.a, b.updateCopy ? m.a : (b.cleanSmall ? m.b : m.a), append);
}
template <bool kTap16, int kGroup, bool kMaskFree>   // (kMaskFree: always false, as clean_args says)
__global__ __launch_bounds__(256) void k_obj_clean_runs(const ObjBatch b) { clean_runs_body<kTap16, kGroup, kMaskFree>(obj_clean_args(b, b.m[blockIdx.z], 0)); }
template <bool kTap16, int kGroup, bool kMaskFree>
__global__ __launch_bounds__(256) void k_obj_clean_small_flags(const ObjBatch b) {
    clean_small_flags_body<kTap16, kGroup, kMaskFree>(obj_clean_args(b, b.m[blockIdx.z], b.cleanSmall ? 0 : 1));
}
__global__ __launch_bounds__(256) void k_obj_clean_small_compact(const ObjBatch b) { clean_small_compact_body(obj_clean_args(b, b.m[blockIdx.z], b.cleanSmall ? 0 : 1)); }
// The prediction of one model of the batch.  (f by value, in functions of their own: a kernel that hands its argument struct to the builders by
// reference itself addresses everything it reaches through that struct as flat memory -- flat_load / flat_store where these kernels have
// global_load / global_store)
__device__ __forceinline__ void obj_splat_scatter(const PassFrame f, const PassModel& m, int dense) {
    // (both forms write the same keys: the z-test is a minimum)
    if (dense) sprite_scatter_body<1, true>(predict_view(f, m), 0u, m.scr.keys, true);
    else sprite_scatter_body<4, true>(predict_view(f, m), 0u, m.scr.keys, true);
}
__device__ __forceinline__ void obj_splat_resolve(const PassFrame f, const PassModel& m) { splat_resolve_body(predict_view(f, m), m.scr.keys, pred_out(f, m)); }
__global__ __launch_bounds__(256) void k_obj_splat_scatter(const ObjBatch b) { obj_splat_scatter(b, b.m[blockIdx.z], b.denseSprites); }
__global__ __launch_bounds__(256) void k_obj_splat_resolve(const ObjBatch b) { obj_splat_resolve(b, b.m[blockIdx.z]); }
__global__ void k_obj_frame_advance(const ObjBatch b) {
    const PassModel& m = b.m[blockIdx.z];
    frame_advance_body(m.frame, b.W, b.H, m.host_frame, m.pose, b.bg_pose, m.log_slot);
}

void launch_obj_fuse_clean(const ObjBatch& b, int blocks, int clean_blocks, hipStream_t s, int compact_blocks) {
    const int P = b.W * b.H;
    const dim3 surfels(blocks, 1, b.n), pixels((P + 255) / 256, 1, b.n), compact(clean_blocks, 1, b.n);
    const int per_wave = b.fuseLanes == 4 ? 16 : 64;
    const dim3 cands(((b.W + 1) / 2 + per_wave - 1) / per_wave, ((b.H + 1) / 2 + 3) / 4, b.n);
    hipLaunchKernelGGL(k_obj_index_scatter, surfels, dim3(256), 0, s, b);
    hipLaunchKernelGGL(k_obj_index_resolve, pixels, dim3(256), 0, s, b);
    if (b.fuseLanes == 4) hipLaunchKernelGGL(k_obj_fuse_data<4>, cands, dim3(256), 0, s, b);
    else hipLaunchKernelGGL(k_obj_fuse_data<1>, cands, dim3(256), 0, s, b);
    if (b.updateCopy) {
        hipLaunchKernelGGL(k_obj_fuse_update_copy, surfels, dim3(256), 0, s, b);
    } else {
        hipLaunchKernelGGL(k_obj_fuse_update, dim3(cand_blocks(b.W, b.H), 1, b.n), dim3(256), 0, s, b);
        hipLaunchKernelGGL(k_obj_index_scatter, surfels, dim3(256), 0, s, b);   // predictIndices after fuse (MaskFusion.cpp:556): the same pass on the updated buffer
    }
    hipLaunchKernelGGL(k_obj_index_resolve_packed, dim3(resolve_tiles(b.W, b.H), 1, b.n), dim3(256), 0, s, b);
    // two-launch form src -> dst, or (big models) the buffer's own surfels in place, run by run -- an object model's launch visits every run: its
    // bounding box is the box of ALL its drawn surfels -- and then the frame's candidates appended by the two-launch form
    const dim3 flags(compact_blocks, 1, b.n);
    const bool tap16 = b.depthT != nullptr;    // the 16-byte tap (the resolve pass above wrote it with each model's own threshold and tick)
    if (!b.cleanSmall) MF_LAUNCH_CLEAN(k_obj_clean_runs, false, tap16, b.cleanTapGroup, false, compact, s, b);
    MF_LAUNCH_CLEAN(k_obj_clean_small_flags, false, tap16, b.cleanTapGroup, false, flags, s, b);
    hipLaunchKernelGGL(k_obj_clean_small_compact, dim3(compact_blocks, 1, b.n), dim3(256), 0, s, b);
}
void launch_obj_predict_advance(const ObjBatch& b, int blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_obj_splat_scatter, dim3(blocks, 1, b.n), dim3(256), 0, s, b);
    hipLaunchKernelGGL(k_obj_splat_resolve, dim3((b.W + 63) / 64, (b.H + 3) / 4, b.n), dim3(256), 0, s, b);
    hipLaunchKernelGGL(k_obj_frame_advance, dim3(1, 1, b.n), dim3(64), 0, s, b);
}

}  // namespace mf
