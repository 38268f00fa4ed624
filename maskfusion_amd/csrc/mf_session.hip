// mf_session.hip -- the kernels of a saved session (mf_session_save / mf_session_load / mf_state_digest, mf_session.inl; DESIGN.md "Sessions").
// No upstream twin: the reference keeps a run's state in one process.
//
//   k_session_pack          a buffer's live surfels in download order (mf_download_map: the runs in order, each run's first len slots; a dense
//                           buffer: slots [0, count)) -> 48-byte interleaved records {pos + conf | colour, unused, initTime, lastTime | normal +
//                           radius} in a staging block.  Reads the buffer, its table and the run offsets; writes the staging block only.
//   k_session_unpack        the inverse: records -> the three streams of a DENSE buffer, slots [first, first + n)
//   k_state_digest          one 64-bit word over a block of bytes taken as little-endian 32-bit words w_0 .. w_{n-1} (the tail zero-padded):
//                               D = sum_i (uint64(w_i) + 1) * (2 i + 1)   mod 2^64
//                           Integer arithmetic: the same word under any reduction order.  (w + 1) * (2 i + 1) is a bijection of w for every i (an
//                           odd factor is invertible mod 2^64), so a change of one word always changes D.
//   k_state_digest_surfels  the same word over the records k_session_pack WOULD write for the buffer -- word 12 o + 4 k + c is component c of stream
//                           k of the surfel with ordinal o --, read from the streams through the same ordinal -> slot computation: a dense buffer
//                           and a run-structured one that hold the same surfels give the same word, and nothing is staged.
//
// Every global access is 16 bytes per lane.  Pack: a workgroup takes 256 consecutive ordinals; lane t reads the three float4 of ordinal t (inside
// a run consecutive lanes read consecutive float4 of each stream), the 768 float4 go through LDS, and the workgroup writes them as 3 x 256
// consecutive float4.  Unpack mirrors it.  Both are streaming gathers without reuse: three read streams, one write stream.
#pragma clang fp contract(off)

#include <cstdint>
#include <cstring>

#include "mf_internal.h"

namespace mf {

namespace {

constexpr int kSessThreads = 256;

// slot of the live surfel with ordinal o (download order).  runs == 0: a dense buffer, slot o.  Else the run r with offs[r] <= o < offs[r + 1]
// (offs: k_run_offsets; an empty run has offs[r] == offs[r + 1] and is never chosen) and the slot o - offs[r] behind its start.
// The caller keeps o below offs[runs].
__device__ __forceinline__ int ordinal_slot(const Surfels& s, int runs, const int* __restrict__ offs, int o) {
    if (runs <= 0) return o;
    int lo = 0, hi = runs;                 // offs[lo] <= o < offs[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= o) lo = mid; else hi = mid;
    }
    return run_start(s.box, lo) + (o - offs[lo]);
}

__device__ __forceinline__ unsigned long long digest_term(uint32_t w, unsigned long long i) { return ((unsigned long long)w + 1ull) * (2ull * i + 1ull); }
__device__ __forceinline__ unsigned long long digest_term4(float4 v, unsigned long long i) {
    return digest_term(__float_as_uint(v.x), i) + digest_term(__float_as_uint(v.y), i + 1) + digest_term(__float_as_uint(v.z), i + 2) +
           digest_term(__float_as_uint(v.w), i + 3);
}
// wavefront shuffle reduction -> LDS -> one 64-bit atomic add per workgroup
__device__ __forceinline__ void digest_commit(unsigned long long acc, unsigned long long* s_w, unsigned long long* __restrict__ word) {
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (int w = 0; w < kSessThreads / 64; ++w) sum += s_w[w];
        if (sum) atomicAdd(word, sum);
    }
}

}  // namespace

// ordinals [first, first + n) -> out[0, 3 n).  The host keeps first + n within the buffer's live count (launch_run_offsets' total).
__global__ __launch_bounds__(kSessThreads) void k_session_pack(Surfels s, const FrameDev* __restrict__ frame, const int* __restrict__ offs, int first, int n,
                                                              float4* __restrict__ out) {
    __shared__ float4 tile[3 * kSessThreads];
    const int runs = frame->runs;
    const int t = (int)threadIdx.x, o0 = (int)blockIdx.x * kSessThreads;
    const int m = min(kSessThreads, n - o0);
    if (t < m) {
        const int slot = ordinal_slot(s, runs, offs, first + o0 + t);
        const bool ok = slot >= 0 && slot < s.cap;     // (a table names slots of its own buffer only; never read past it)
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        tile[3 * t] = ok ? s.pc[slot] : z;
        tile[3 * t + 1] = ok ? s.ct[slot] : z;
        tile[3 * t + 2] = ok ? s.nr[slot] : z;
    }
    __syncthreads();
    float4* dst = out + (size_t)o0 * 3;
    for (int j = t; j < 3 * m; j += kSessThreads) dst[j] = tile[j];
}

// rec[0, 3 n) -> slots [first, first + n) of dst's streams (first + n <= dst.cap: the host's check)
__global__ __launch_bounds__(kSessThreads) void k_session_unpack(const float4* __restrict__ rec, int n, Surfels dst, int first) {
    __shared__ float4 tile[3 * kSessThreads];
    const int t = (int)threadIdx.x, o0 = (int)blockIdx.x * kSessThreads;
    const int m = min(kSessThreads, n - o0);
    const float4* src = rec + (size_t)o0 * 3;
    for (int j = t; j < 3 * m; j += kSessThreads) tile[j] = src[j];
    __syncthreads();
    const int slot = first + o0 + t;
    if (t < m && slot < dst.cap) {
        dst.pc[slot] = tile[3 * t];
        dst.ct[slot] = tile[3 * t + 1];
        dst.nr[slot] = tile[3 * t + 2];
    }
}

// *word += the digest terms of `bytes` bytes at data (16-byte aligned), whose first word has index first_word; any grid
__global__ __launch_bounds__(kSessThreads) void k_state_digest(const uint32_t* __restrict__ data, unsigned long long bytes, unsigned long long first_word,
                                                              unsigned long long* __restrict__ word) {
    __shared__ unsigned long long s_w[kSessThreads / 64];
    const unsigned long long n_words = bytes / 4ull, n_vec = n_words / 4ull;
    const unsigned long long gid = (unsigned long long)blockIdx.x * kSessThreads + threadIdx.x, stride = (unsigned long long)gridDim.x * kSessThreads;
    const uint4* vec = reinterpret_cast<const uint4*>(data);
    unsigned long long acc = 0;
    for (unsigned long long v = gid; v < n_vec; v += stride) {
        const uint4 q = vec[v];
        const unsigned long long i = first_word + 4ull * v;
        acc += digest_term(q.x, i) + digest_term(q.y, i + 1) + digest_term(q.z, i + 2) + digest_term(q.w, i + 3);
    }
    for (unsigned long long i = 4ull * n_vec + gid; i < n_words; i += stride) acc += digest_term(data[i], first_word + i);
    if (gid == 0 && (bytes & 3ull)) {      // the last, partial word: its missing bytes are zero
        const uint8_t* b = reinterpret_cast<const uint8_t*>(data) + 4ull * n_words;
        uint32_t w = 0;
        for (unsigned k = 0; k < (unsigned)(bytes & 3ull); ++k) w |= (uint32_t)b[k] << (8 * k);
        acc += digest_term(w, first_word + n_words);
    }
    digest_commit(acc, s_w, word);
}

// *word += the digest of the records of the buffer's live surfels (*total of them, at most s.cap); any grid
__global__ __launch_bounds__(kSessThreads) void k_state_digest_surfels(Surfels s, const FrameDev* __restrict__ frame, const int* __restrict__ offs,
                                                                      const int* __restrict__ total, unsigned long long* __restrict__ word) {
    __shared__ unsigned long long s_w[kSessThreads / 64];
    const int runs = frame->runs, n = min(*total, s.cap);
    unsigned long long acc = 0;
    for (int o = (int)(blockIdx.x * kSessThreads + threadIdx.x); o < n; o += (int)(gridDim.x * kSessThreads)) {
        const int slot = ordinal_slot(s, runs, offs, o);
        if (slot < 0 || slot >= s.cap) continue;
        const unsigned long long i = 12ull * (unsigned long long)o;
        acc += digest_term4(s.pc[slot], i) + digest_term4(s.ct[slot], i + 4) + digest_term4(s.nr[slot], i + 8);
    }
    digest_commit(acc, s_w, word);
}

void launch_session_pack(Surfels s, const FrameDev* frame, const int* offs, int first, int n, float4* out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_session_pack, dim3((unsigned)((n + kSessThreads - 1) / kSessThreads)), dim3(kSessThreads), 0, st, s, frame, offs, first, n, out);
}
void launch_session_unpack(const float4* rec, int n, Surfels dst, int first, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_session_unpack, dim3((unsigned)((n + kSessThreads - 1) / kSessThreads)), dim3(kSessThreads), 0, st, rec, n, dst, first);
}
static unsigned digest_grid(unsigned long long lanes) {
    const unsigned long long b = (lanes + kSessThreads - 1) / kSessThreads;
    return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}
void launch_state_digest(const void* data, uint64_t bytes, uint64_t first_word, unsigned long long* word, hipStream_t st) {
    if (bytes == 0) return;
    hipLaunchKernelGGL(k_state_digest, dim3(digest_grid(bytes / 16 + 1)), dim3(kSessThreads), 0, st, reinterpret_cast<const uint32_t*>(data),
                       (unsigned long long)bytes, (unsigned long long)first_word, word);
}
void launch_state_digest_surfels(Surfels s, const FrameDev* frame, const int* offs, const int* total, int expected, unsigned long long* word, hipStream_t st) {
    hipLaunchKernelGGL(k_state_digest_surfels, dim3(digest_grid((unsigned long long)(expected > 0 ? expected : 1))), dim3(kSessThreads), 0, st, s, frame,
                       offs, total, word);
}
// the same word on the host (the sections that live there, and what mf_session_info checks without a GPU)
uint64_t state_digest_host(const void* data, uint64_t bytes, uint64_t first_word) {
    const uint8_t* b = static_cast<const uint8_t*>(data);
    uint64_t d = 0;
    const uint64_t n_words = bytes / 4;
    for (uint64_t i = 0; i < n_words; ++i) {
        uint32_t w;
        memcpy(&w, b + 4 * i, 4);
        d += ((uint64_t)w + 1u) * (2u * (first_word + i) + 1u);
    }
    if (bytes & 3u) {
        uint32_t w = 0;
        for (unsigned k = 0; k < (unsigned)(bytes & 3u); ++k) w |= (uint32_t)b[4 * n_words + k] << (8 * k);
        d += ((uint64_t)w + 1u) * (2u * (first_word + n_words) + 1u);
    }
    return d;
}

}  // namespace mf
