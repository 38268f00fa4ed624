// mf_splat.hip -- tiled splat prediction (ModelProjection::combinedPredict, Core/Model/ModelProjection.cpp:187-268 +
// Core/Shaders/splat.vert, combo_splat.frag) and tiled GlobalProjection: the sprite set-up, ray and pixel test of
// mf_sprite_device.h -- the ones k_splat_scatter / k_splat_resolve in mf_surfel.hip and k_global_scatter in mf_segment.hip run
// (those stay as the executable specification: tests compare the forms bit for bit) --, organised so that the z-test happens in LDS.
//
// Why: the scatter form issues one 64-bit global atomicMin per covered pixel (4.3 M per VGA frame at 270 k surfels).
// Device-scope atomics are performed memory-side (rocprofv3: TCC_HIT ~ 0, every request a miss; a line touched by an
// atomic is dropped from L2, so a read-before-atomic filter costs as much as the atomic) and the kernel sat at 81 us,
// issue-stalled (SQ_WAIT_INST_ANY 68 % of wave cycles).  Here surfels are binned to 16x16-pixel tiles (two passes with
// LDS histograms: ~13 k global atomics instead of 4.3 M), one workgroup per tile runs the z-test with ds_min_u64 on a 2 KB
// LDS tile, and the winner's attributes are written straight to the prediction maps -- no key buffer, no resolve pass.
#pragma clang fp contract(off)

#include "mf_internal.h"
#include "mf_device.h"
#include "mf_sprite_device.h"
#include "mf_rgbd_device.h"
#include "mf_bilateral_device.h"
#include "mf_frame_pyramid_device.h"
#include "mf_model_pyramid_device.h"

namespace mf {

constexpr int kTile = 16;                // tile width in pixels
constexpr int kTileHMax = 32;            // the tallest tile: the height is a launch parameter ("tileHeight", SplatTuning::tile_h; 24 since round 6).
                                         // 1 200 workgroups of 16 x 16 tiles at VGA are more than the 1 024 that are resident at once; 800 of 16 x 24 are one
                                         // round: prediction stage 53.0 -> 50.8 us at VGA, the 1280 x 960 frame 861 -> 848 us (profiles/r06zj_ab.txt); 16 x 32: 52.6 us at VGA, 843 us at
                                         // 1280 x 960, configs[4] unchanged (r06zk_ab.txt)
constexpr int kBinThreads = 1024;
constexpr int kMaxTiles = 8192;          // bounds the LDS histograms (VGA: 1200 tiles, 1280x960: 4800); larger images use the scatter form

struct TileStamps { unsigned long long t[8]; };   // "splatProfile": shader-clock stamps of a tile workgroup's thread 0 (by reference + constant
                                                  // indices: an array handed over as a pointer lives in scratch memory, for every launch)

// The three knobs of SplatTuning.  Their legal values are the rows of mf_params.inl (mf_set_param refuses everything else); what follows only guards
// the launches against a SplatTuning filled in by hand: anything else takes the default.
// lanes that share one sprite in the tile z-test (mf_set_param "spriteLanes"): an A/B switch for measurements, per context
// (SplatTuning travels with the launch; rounds 2-3 kept both knobs in process-wide statics that one context's setting changed for all)
int splat_sprite_lanes(int n) { return (n == 1 || n == 2 || n == 8 || n == 16) ? n : 4; }
// threads per tile workgroup ("tileThreads"): a tile has 256 pixels, the threads beyond them only walk the sprite list.
// 1200 tiles of 256 threads are 4.7 wavefronts per SIMD on 256 CUs -- too few to hide the list's dependent gathers and the division
// chain of the pixel test (tools/splat_prof.py: a tile workgroup lives ~32 k cycles, ~4 k of them issuing)
// Measured (profiles/r03k_*, prediction stage incl. binning): 256 threads 62.6 us, 512 threads 58.0 us, 1024 threads 65.9 us (4 lanes per
// sprite each) -- 512 is the default.
int splat_tile_threads(int n) { return (n == 256 || n == 320 || n == 384 || n == 1024) ? n : 512; }
// tile height ("tileHeight"): that many rows of 16 pixels; the tile's pixels need a thread each
int splat_tile_height(int h) { return (h == 16 || h == 20 || h == 32) ? h : 24; }

// The launch shape of the tile passes (mf_internal.h)
TileShape splat_tile_shape(int W, int H, SplatTuning tune) {
    TileShape t;
    t.tileH = splat_tile_height(tune.tile_h);
    t.tilesX = (W + kTile - 1) / kTile; t.tilesY = (H + t.tileH - 1) / t.tileH;
    t.lanes = splat_sprite_lanes(tune.sprite_lanes);
    t.threads = std::max(splat_tile_threads(tune.tile_threads), ((kTile * t.tileH + 63) / 64) * 64);   // the tile's pixels need a thread each
    t.fits = t.tilesX * t.tilesY <= kMaxTiles;
    return t;
}

// What the binning pass writes and the tile pass of the same view reads
struct BinArgs {
    SpriteView v;         // (v.frame->pad[1]: the overflow flag)
    int tilesX, tilesY, tileH;
    int* tile_count;      // [tiles]  zero on entry (each tile workgroup re-zeroes its own counter when it is done)
    int* entries;         // [tiles][tile_cap]
    int tile_cap;
    float4* rec0; float4* rec1; short4* bbox;   // [surfels] sprite set-up kept for the tile pass: {h, r^2}, {n, h.n}, pixel box
    const int* vis_list; const int* vis_count;  // nullptr: every surfel; else the runs of v.src (Surfels::box) k_cull listed -- no other run can draw
};

// Binning in one pass: every tile owns a fixed slice of `entries`, so no scan is needed.  A 1024-thread workgroup counts
// its entries per tile in LDS, reserves a contiguous range per touched tile with ONE global atomicAdd (~13 k per frame
// instead of one global atomic per covered pixel), then hands out slots inside the range with LDS atomics.  The order of
// a tile's list is not deterministic; the z-test that consumes it is order independent.
// (the workgroup body: k_splat_bin below runs it on 1024 threads, k_bin_bilateral -- beside the next frame's depth filter -- on 256.  s_mem: 2 nt
// ints of LDS; block / nblocks: this workgroup's index among the nblocks workgroups that share the rounds)
template <int kThreads>
__device__ __forceinline__ void splat_bin_body(const BinArgs& a, int* s_mem, const int block, const int nblocks) {
    const int nt = a.tilesX * a.tilesY;
    int* s_cnt = s_mem;           // [nt] this workgroup's entries per tile, then the start of its reserved range
    int* s_fill = s_mem + nt;     // [nt] slots handed out
    const int n = a.v.frame->phys;      // device-resident: the grid is fixed and walks the buffer in chunks of 2048 slots
    // by runs: the listed ones (k_cull), or every run of the buffer's table; a dense buffer without a table: slot by slot
    const int table_runs = a.v.frame->runs;
    const bool by_runs = a.vis_list != nullptr || table_runs > 0;
    const int nruns = a.vis_list ? *a.vis_count : table_runs;
    const float time = (float)a.v.frame->tick;
    float Ri[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Ri[q] = a.v.pose->Ri[q];
    const float3 ti = f3(a.v.pose->ti[0], a.v.pose->ti[1], a.v.pose->ti[2]);
  // a round = 2 kThreads surfel slots (2048 in k_splat_bin): consecutive surfels of the buffer, or -- with a visibility list -- the next 2 kThreads / kRun listed runs
  constexpr int kRunsPerRound = 2 * kThreads / kRun;
  const int rounds = by_runs ? (nruns + kRunsPerRound - 1) / kRunsPerRound : (n + 2 * kThreads - 1) / (2 * kThreads);
  for (int chunk = block; chunk < rounds; chunk += nblocks) {
    for (int t = threadIdx.x; t < nt; t += kThreads) { s_cnt[t] = 0; s_fill[t] = 0; }
    __syncthreads();
    // 2 surfels per thread; their sprite boxes stay in registers between the two phases
    int idx[2]; short4 bb[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        int i = (chunk * 2 + r) * kThreads + threadIdx.x;
        if (by_runs) {
            const int slot = r * kThreads + (int)threadIdx.x, v = chunk * kRunsPerRound + slot / kRun;
            i = n;
            if (v < nruns) {
                const int run = a.vis_list ? a.vis_list[v] : v;
                const int beg = run_start(a.v.src.box, run), len = run_len(a.v.src.box, run);
                if (slot % kRun < len) i = beg + slot % kRun;
            }
        }
        idx[r] = i;
        bb[r] = make_short4(1, 0, 1, 0);
        if (i < n) {
            SplatSetup su;
            if (splat_setup(a.v, i, time, Ri, ti, su)) {
                bb[r] = make_short4((short)su.px0, (short)su.px1, (short)su.py0, (short)su.py1);
                // the tile pass meets this surfel ~1.8 times (once per overlapped tile): it reads the set-up instead of
                // repeating its ~300 instructions (ten IEEE divisions) each time
                a.rec0[i] = make_float4(su.h.x, su.h.y, su.h.z, su.sqrRad);
                a.rec1[i] = make_float4(su.nrm.x, su.nrm.y, su.nrm.z, su.pn);
                for (int ty = su.py0 / a.tileH; ty <= su.py1 / a.tileH; ++ty)
                    for (int tx = su.px0 / kTile; tx <= su.px1 / kTile; ++tx) atomicAdd(&s_cnt[ty * a.tilesX + tx], 1);
            }
            a.bbox[i] = bb[r];   // also for surfels that draw nothing (empty box): the overflow path of the tile pass scans every box
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nt; t += kThreads)
        if (s_cnt[t]) s_cnt[t] = atomicAdd(&a.tile_count[t], s_cnt[t]);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (bb[r].x > bb[r].y) continue;
        for (int ty = bb[r].z / a.tileH; ty <= bb[r].w / a.tileH; ++ty)
            for (int tx = bb[r].x / kTile; tx <= bb[r].y / kTile; ++tx) {
                const int t = ty * a.tilesX + tx;
                const int slot = s_cnt[t] + atomicAdd(&s_fill[t], 1);
                // a full list is not an error and drops nothing: tile_count keeps counting, and a tile whose count exceeds its
                // slice scans the sprite boxes of the whole map instead of its list (k_splat_tile); pad[1] only records that it happened
                if (slot < a.tile_cap) a.entries[(size_t)t * a.tile_cap + slot] = idx[r];
                else a.v.frame->pad[1] = 1;
            }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBinThreads) void k_splat_bin(const BinArgs a) {
    extern __shared__ int s_mem[];
    splat_bin_body<kBinThreads>(a, s_mem, (int)blockIdx.x, (int)gridDim.x);
}

// The binning pass of frame t's prediction and the depth filter of frame t + 1 in ONE launch ("fusedBinFilter"; mf_frame.inl: enqueue_fused_head).
// The two are independent -- the binning pass reads the cleaned map and the pose, the filter the new depth image -- and complement each other: the
// filter is VALU-bound, the binning pass a stream plus LDS atomics that, at 2048 surfels per workgroup, keeps half the compute units busy.  The
// workgroups have the filter's 256 threads: nbin of them run splat_bin_body on rounds of 512 surfels, the others bilateral_body on one 64 x 4
// tile each -- the bodies of k_splat_bin and k_bilateral.  (The order of a tile's list is no more deterministic here than there; what the tile
// pass makes of it does not depend on the order.)  Both halves count in multiples of 8 workgroups and are dealt out in turns of 8 where the launch
// is not resident at once (a Bresenham walk, as k_bilateral_model_pyramid's), so that a filter tile keeps the XCD k_bilateral's index gives it
// (xcd_contiguous_tile) and both halves are in flight from the first round on.
// (1024-thread workgroups with four filter tiles each -- the binning pass as it stands -- were measured first: 31.6 us against 14.1 + 15.9 for the
// two launches; 300 filter workgroups of four tiles on 256 compute units leave the last ones with twice the average load.  DESIGN.md)
constexpr int kBinFilterThreads = 256;
__global__ __launch_bounds__(kBinFilterThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_bin_bilateral(const BinArgs a, int nbin, int interleave,
                                                                                                               const float* __restrict__ depth,
                                                                                                               float* __restrict__ out, int W, int H) {
    extern __shared__ int s_mem[];
    const int groups = (int)gridDim.x >> 3, gfil = groups - (nbin >> 3), g = (int)blockIdx.x >> 3, lane = (int)blockIdx.x & 7;
    int before, after;   // filter groups in front of group g / of group g + 1
    if (interleave) { before = (int)(((long long)g * gfil) / groups); after = (int)(((long long)(g + 1) * gfil) / groups); }
    else { before = g < (nbin >> 3) ? 0 : g - (nbin >> 3); after = g < (nbin >> 3) ? 0 : before + 1; }
    if (after == before) { splat_bin_body<kBinFilterThreads>(a, s_mem, ((g - before) << 3) + lane, nbin); return; }
    bilateral_body(depth, out, W, H, reinterpret_cast<float*>(s_mem), (before << 3) + lane, (int)threadIdx.x, true);
}

struct TileArgs {
    BinArgs b;                       // the binning pass's arguments: the view, the tile shape, the lists and records it wrote
    PredOut out;
    int advance; FrameAdvance adv;   // advance != 0: the last workgroup also runs the end-of-frame bookkeeping (k_frame_advance)
    unsigned long long* prof;        // optional ("splatProfile"): [tiles][8] shader-clock stamps of thread 0 + the tile's list length
    float* vm[3]; float* nm[3];      // optional ("tilePyramid"; vm[0] == nullptr: off): the model-side pyramid's planes -- every tile workgroup also writes their texels
    int tile_wgs;                    // workgroups of the launch that run the tile pass (the padded tile count); any behind them build the frame pyramid
};

// The z-test of one tile in LDS, shared by the prediction (the key's low word = surfel index) and the global projection (= payload:
// model order / id): rays of the tile's pixels, the tile's sprite list (or, after a list overflow, every sprite box of the map),
// ds_min_u64 per covered pixel.  On return s_key[pixel of the tile] holds the winning key (all threads have passed a barrier).
template <bool kIndexKey, int kSpriteLanes>
__device__ __forceinline__ void tile_ztest(const BinArgs& a, int tile, unsigned payload, unsigned long long* s_key, float4* s_ray, int* s_range, bool prof,
                                           TileStamps& stamp) {
    const int tx0 = (tile % a.tilesX) * kTile, ty0 = (tile / a.tilesX) * a.tileH;
    const float4* __restrict__ const rec0 = a.rec0; const float4* __restrict__ const rec1 = a.rec1; const short4* __restrict__ const bbox = a.bbox;   // (read only here)
    if ((int)threadIdx.x < kTile * a.tileH) {
    s_key[threadIdx.x] = kEmptyKey;
    {   // the viewing ray of every pixel of the tile, once (combo_splat.frag:40-42); the per-surfel loops below re-used to
        // spend two thirds of their instructions recomputing it (two divisions + a normalisation per covered pixel)
        const float3 l = sprite_ray(tx0 + (int)(threadIdx.x & (kTile - 1)), ty0 + (int)(threadIdx.x >> 4), a.v.k);
        s_ray[threadIdx.x] = make_float4(l.x, l.y, l.z, 0.f);
    }
    }
    if (threadIdx.x == 0) {
        s_range[0] = a.tile_count[tile];
        a.tile_count[tile] = 0;   // consumed: the next binning pass starts from zero
    }
    __syncthreads();
    if (prof) { stamp.t[1] = __builtin_amdgcn_s_memtime(); stamp.t[6] = (unsigned long long)s_range[0]; }
    const bool overflow = s_range[0] > a.tile_cap;   // more sprites than list slots (the reference has no such limit): scan every box
    // (after an overflow: every surfel whose sprite box the binning pass wrote -- the runs of the visibility list, every run of the table, or
    // -- a dense buffer without a table -- every slot)
    // (looked at after an overflow only: the common path waits for nothing but its list)
    const int table_runs = overflow ? a.v.frame->runs : 0;
    const bool by_runs = a.vis_list != nullptr || table_runs > 0;
    const int cnt = overflow ? (by_runs ? (a.vis_list ? *a.vis_count : table_runs) * kRun : a.v.frame->count) : s_range[0];
    const int* __restrict__ list = a.entries + (size_t)tile * a.tile_cap;
    auto entry = [&](int e) -> int {
        if (!overflow) return list[e];
        if (!by_runs) return e;
        const int run = a.vis_list ? a.vis_list[e / kRun] : e / kRun;
        return e % kRun < run_len(a.v.src.box, run) ? run_start(a.v.src.box, run) + e % kRun : -1;
    };
    // kSpriteLanes neighbouring lanes share one sprite and take every kSpriteLanes-th pixel of its clipped box (with one lane per sprite a
    // wavefront runs as long as its largest box).  The lanes read the same list entry / records (one request) and the z-test is order
    // independent, so the keys are the same bits.  Measured on MI355X (profiles/r03h_*): prediction stage 65.5 us with 1 lane,
    // 62.2 / 62.6 with 2 / 4, 66.3 with 8, 81.4 with 16 -- the boxes are small (4.3 px a side on the bench stream), and the pass is half
    // VALU (two IEEE divisions' worth per pixel test), half gather latency; 4 is the default.
    constexpr int kLX = kSpriteLanes >= 8 ? 4 : (kSpriteLanes >= 2 ? 2 : 1), kLY = kSpriteLanes / kLX;
    const int sub = threadIdx.x & (kSpriteLanes - 1), sx = sub % kLX, sy = sub / kLX;
    // Software pipeline over the list (round 4).  An entry costs three DEPENDENT gathers -- list[e] -> bbox[i] -> rec0[i], rec1[i] -- and the
    // in-kernel stamps of round 3 (tools/splat_prof.py) showed a tile workgroup issuing for ~4 k of its ~32 k cycles: it waits.  Every round
    // now first issues the loads of LATER rounds -- the list entry two rounds ahead, the box and the two records of the next round's sprite
    // (every listed sprite overlaps the tile, so its records are always needed) -- and only then tests the sprite whose data arrived during
    // the previous round: one memory latency per round, overlapped with the pixel tests, instead of three in a row.  Same keys, bit for bit.
    const int stride = (int)blockDim.x / kSpriteLanes;   // blockDim.x = 256, 512 or 1024 ("tileThreads")
    const int e0 = threadIdx.x / kSpriteLanes;
    const short4 kNoBox = make_short4(1, 0, 1, 0);
    int i0 = e0 < cnt ? entry(e0) : -1;
    int i1 = e0 + stride < cnt ? entry(e0 + stride) : -1;
    short4 bb0 = i0 >= 0 ? bbox[i0] : kNoBox;
    float4 r0 = i0 >= 0 ? rec0[i0] : make_float4(0, 0, 0, 0), r1 = i0 >= 0 ? rec1[i0] : make_float4(0, 0, 0, 0);
    for (int e = e0; e < cnt; e += stride) {
        const int i = i0;
        const short4 bb = bb0;
        const float4 c0 = r0, c1 = r1;
        // loads of the rounds to come (nothing below depends on them)
        const int e2 = e + 2 * stride;
        const int i2 = e2 < cnt ? entry(e2) : -1;
        if (i1 >= 0) { bb0 = bbox[i1]; r0 = rec0[i1]; r1 = rec1[i1]; } else bb0 = kNoBox;
        i0 = i1; i1 = i2;
        const int x0 = max((int)bb.x, tx0), x1 = min((int)bb.y, tx0 + kTile - 1);
        const int y0 = max((int)bb.z, ty0), y1 = min((int)bb.w, ty0 + a.tileH - 1);
        if (x0 > x1 || y0 > y1) continue;
        SplatSetup su;
        su.h = f3(c0.x, c0.y, c0.z); su.sqrRad = c0.w; su.nrm = f3(c1.x, c1.y, c1.z); su.pn = c1.w;
        // the kSpriteLanes lanes of a sprite form a kLX x kLY block that strides over the box: two plain nested loops (a flat pixel counter
        // needed a wrap-around loop per pixel), and the next pixel's ray is on its way from LDS while this one is tested
        for (int py = y0 + sy; py <= y1; py += kLY) {
            const int row = (py - ty0) * kTile - tx0;
            int px = x0 + sx;
            float4 nxt = s_ray[row + min(px, x1)];
            for (; px <= x1; px += kLX) {
                const int lp = row + px;
                const float4 r4 = nxt;
                nxt = s_ray[row + min(px + kLX, x1)];
                float z;
                if (!sprite_covers(su, f3(r4.x, r4.y, r4.z), z)) continue;
                atomicMin(&s_key[lp], sprite_key(z, kIndexKey ? (unsigned)i : payload));   // (looking at s_key before the atomic -- most sprites lose -- was measured: no gain)
            }
        }
    }
    if (prof) stamp.t[2] = __builtin_amdgcn_s_memtime();
    __syncthreads();
    if (prof) stamp.t[3] = __builtin_amdgcn_s_memtime();
}

// Pass 3: one workgroup (512 threads by default, the first 256 own the pixels) per 16x16 tile: LDS z-test over the tile's surfel list, then the fragment outputs
// (combo_splat.frag) of every pixel of the tile.
//
// "tilePyramid" (a.vm set): the workgroup then also writes the three levels of the model-side pyramid for its tile -- what model_pyramid_body
// (mf_model_pyramid.hip) computes WITHOUT fill-in from the prediction maps this workgroup has just written.  Every output of that pyramid depends on one
// aligned 4 x 4 block of level-0 texels, and a tile is a whole number of such blocks: level 0 goes out from the registers that hold the pixel, the
// pixel's copyMaps value is staged in the z-test's LDS (free by now: rays in s_ray, keys in s_key -- a thread overwrites only the slot it has read),
// and behind the barrier the workgroup takes anyway one thread per level-1 texel, a DPP quad per level-2 texel, runs model_pyramid_down
// (mf_model_pyramid_device.h) -- the function model_pyramid_body calls.  Whether the tracking step fills in is decided by THIS launch's last
// workgroup from the coverage of the whole image, so no tile knows it: a frame whose decision comes out "fill" gets its pyramid rebuilt by the
// fix-up launch behind (k_model_pyramid with PyrArgs::fixup; mf_frame.inl: enqueue_fused_head).
//
// "fusedTilePyramid": workgroups behind the a.tile_wgs tile workgroups build the NEXT frame's pyramid from its filtered depth (frame_pyramid_body,
// mf_frame_pyramid_device.h) -- independent of the tile pass, LDS-tiled and light on VALU, where the tile pass waits for gathers and its workgroups
// live 10 us of a 25 us launch.  The body is written for 256 threads: a workgroup of 512 (1024) takes two (four) pyramid tiles, each 256 threads with
// an LDS slice of their own; they meet only in the body's barriers.  A pyramid workgroup takes no ticket.
constexpr int kTilePoolFloat4 = (4 * kFpLdsFloats + 3) / 4;   // LDS of a workgroup: rays + keys of a tile (768 float4), or four pyramid tiles' depths
static_assert(kTilePoolFloat4 >= kTile * kTileHMax + kTile * kTileHMax / 2, "the pool holds a tile's rays and keys");
template <int kSpriteLanes>
// (eight wavefronts per SIMD, as before the epilogue: left alone the compiler takes 75 registers for it and a compute unit holds three 512-thread
// workgroups instead of four)
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_splat_tile(const TileArgs a, const FramePyrArgs fp) {
    __shared__ float4 s_pool[kTilePoolFloat4];
    __shared__ int s_range[1];
    __shared__ int s_cover;
    if ((int)blockIdx.x >= a.tile_wgs) {
        // pyramid tiles of this workgroup: sub-tile `sub` of workgroup j is block (j / 8 * nsub + sub) * 8 + j % 8 of the body's grid -- the index keeps
        // its XCD (a.tile_wgs is a multiple of 8) and the XCD its band of tile rows (xcd_contiguous_tile)
        const int nsub = (int)blockDim.x >> 8, sub = (int)threadIdx.x >> 8, j = (int)blockIdx.x - a.tile_wgs;
        const bool has = sub < nsub;   // (a workgroup of 320 / 384 threads: the threads behind the first 256 belong to no tile)
        frame_pyramid_body<false>(fp, reinterpret_cast<float*>(s_pool) + (has ? sub : 0) * kFpLdsFloats, ((((j >> 3) * nsub + sub) << 3) + (j & 7)),
                                  (int)threadIdx.x & 255, has);
        return;
    }
    const BinArgs& bin = a.b;
    const SpriteView& v = bin.v;
    const PredOut& o = a.out;
    float4* const s_ray = s_pool;
    unsigned long long* const s_key = reinterpret_cast<unsigned long long*>(s_pool + kTile * kTileHMax);
    // XCD k draws the k-th contiguous eighth of the tile list (mf_device.h): a sprite overlaps 1.8 tiles on average, and neighbouring
    // tiles now find its records in the same L2.  The grid is padded to a multiple of 8; a padding workgroup draws nothing but still
    // takes its ticket below.
    const int tile = xcd_contiguous_tile(blockIdx.x, bin.tilesX * bin.tilesY);
    const bool live = tile < bin.tilesX * bin.tilesY;
    const int tx0 = (tile % bin.tilesX) * kTile, ty0 = (tile / bin.tilesX) * bin.tileH;
    const Intr k = v.k;
    if (threadIdx.x == 0) s_cover = 0;   // (ordered before its use by the barriers inside tile_ztest)
    TileStamps stamp;
    const bool prof = a.prof != nullptr && live && threadIdx.x == 0;
    if (prof) {
#pragma unroll
        for (int q = 0; q < 8; ++q) stamp.t[q] = 0;
        stamp.t[0] = __builtin_amdgcn_s_memtime();
    }
    if (live) tile_ztest<true, kSpriteLanes>(bin, tile, 0u, s_key, s_ray, s_range, prof, stamp);
    const int px = tx0 + (threadIdx.x & (kTile - 1)), py = ty0 + (threadIdx.x >> 4);
    int covered = 0;   // this pixel is one of the 20x down-sampled samples of MaskFusion::requiresFillIn and carries a colour
    const bool pyr = a.vm[0] != nullptr;
    // (gathering the winners' records along the tile's COLUMNS and transposing the outputs through the LDS -- what made the index map's resolve
    // twice as fast -- changes nothing here: 61.3 against 60.0 us for the stage, profiles/r05r_ab.txt; a sprite covers ~4 x 4 pixels, neighbouring
    // pixels share their winner either way)
    if (live && (int)threadIdx.x < kTile * bin.tileH && px < v.W && py < v.H) {   // (threads beyond the tile's 256 pixels only helped with the list)
      const int p = py * v.W + px;
      const unsigned long long key = s_key[threadIdx.x];
      float4 v4 = make_float4(0, 0, 0, 0), n4 = v4;
      if (key == kEmptyKey) {
        o.predV[p] = o.predN[p] = make_float4(0, 0, 0, 0);
        o.predImage[p] = make_uchar4(0, 0, 0, 0);
        o.predTime[p] = 0;
        if (o.predGray) o.predGray[p] = 0;
        if (o.fillGray && o.rgb) o.fillGray[p] = intensity_of((float)o.rgb[p * 3], (float)o.rgb[p * 3 + 1], (float)o.rgb[p * 3 + 2]);
      } else {
        const int i = (int)(unsigned)(key & 0xFFFFFFFFull);
        const float z = __uint_as_float((unsigned)(key >> 32));
        const float4 pc = v.src.pc[i], c4 = v.src.ct[i], s4 = v.src.nr[i];
        const float3 n = normalize_gl(mul33(v.pose->Ri, f3(s4.x, s4.y, s4.z)));
        const float fcx = (float)px + 0.5f, fcy = (float)py + 0.5f;
        v4 = make_float4((fcx - k.cx) * z * (1.f / k.fx), (fcy - k.cy) * z * (1.f / k.fy), z, pc.w);  // combo_splat.frag:56
        n4 = make_float4(n.x, n.y, n.z, s4.w);
        o.predV[p] = v4;
        o.predN[p] = n4;
        const int ci = (int)c4.x;
        const uchar4 col = make_uchar4((ci >> 16) & 0xFF, (ci >> 8) & 0xFF, ci & 0xFF, 255);
        o.predImage[p] = col;
        o.predTime[p] = (uint16_t)(unsigned)c4.z;
        if (o.predGray || o.fillGray) {
            const uint8_t gv = intensity_of((float)col.x, (float)col.y, (float)col.z);
            if (o.predGray) o.predGray[p] = gv;
            if (o.fillGray) {
                const bool empty = (col.x == 0 && col.y == 0 && col.z == 0) || o.fillPassthrough != 0;
                o.fillGray[p] = (empty && o.rgb) ? intensity_of((float)o.rgb[p * 3], (float)o.rgb[p * 3 + 1], (float)o.rgb[p * 3 + 2]) : gv;
            }
        }
        // MaskFusion::requiresFillIn (MaskFusion.cpp:630-648): nearest sample of the 20x down-sampled colour prediction
        covered = ((px % 20) == 10 && (py % 20) == 10 && px / 20 < v.W / 20 && py / 20 < v.H / 20 && col.x > 0 && col.y > 0 && col.z > 0) ? 1 : 0;
      }
      if (pyr) {
        // copyMapsKernel of the texel; its flags are the values' own NaNs (vok = !isnan(v.x), nok = !isnan(n.x)), so six floats carry it.  Level 0
        // covers the whole 4 x 4 blocks of the image, as model_pyramid_body's threads do
        const MapPx m = copy_maps_px(v4, n4);
        float Rm[9];   // the model pose, as model_pyramid_body reads it (scalar loads; read again behind the barrier rather than kept across it)
#pragma unroll
        for (int q = 0; q < 9; ++q) Rm[q] = v.pose->R[q];
        const float3 tm = f3(v.pose->t[0], v.pose->t[1], v.pose->t[2]);
        s_ray[threadIdx.x] = make_float4(m.v.x, m.v.y, m.v.z, m.n.x);
        s_key[threadIdx.x] = ((unsigned long long)__float_as_uint(m.n.z) << 32) | (unsigned long long)__float_as_uint(m.n.y);
        if (px < 4 * (v.W >> 2) && py < 4 * (v.H >> 2)) store_tx(a.vm[0], a.nm[0], v.W * v.H, p, m.v, m.vok, m.n, m.nok, Rm, tm);
      }
    }
    // One 64-bit atomic per workgroup carries both its coverage count and its "finished" ticket (the count travels IN the atomic, so
    // the workgroup that draws the last ticket holds the launch's total without any ordering between workgroups).  That workgroup
    // hands the total on: to frame->cover for a stand-alone prediction, or straight into the end-of-frame bookkeeping that used to be
    // its own single-thread launch (k_frame_advance, ~4.7 us per model and frame).  Nothing else in this launch reads what it writes.
    if (prof) {
        stamp.t[4] = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp.t[5] = __builtin_amdgcn_s_memtime();
#pragma unroll
        for (int q = 0; q < 8; ++q) a.prof[(size_t)tile * 8 + q] = stamp.t[q];
    }
    if (covered) atomicAdd(&s_cover, 1);   // at most two such pixels per 16x16 tile
    __syncthreads();
    if (threadIdx.x == 0) {
        const int wg_cover = s_cover;
        const unsigned long long old = atomicAdd(&v.frame->done_cover, (1ull << 32) | (unsigned long long)(unsigned)wg_cover);
        if ((unsigned)(old >> 32) == (unsigned)a.tile_wgs - 1u) {   // (the tile workgroups' tickets: others may share the launch)
            const int cover = (int)(unsigned)(old & 0xFFFFFFFFull) + wg_cover;
            FrameDev* f = v.frame;
            f->done_cover = 0ull;
            if (a.advance) {
                if (a.adv.log_slot) pose_log_entry(v.pose, a.adv.bg_pose, a.adv.log_slot);
                const int rw = v.W / 20, rh = v.H / 20;
                f->pad[0] = f->useFillIn;   // decision the tracking step of THIS frame ran with (mf_get_last_fillin)
                f->useFillIn = ((float)(f->cover + cover) / (float)(rw * rh) < 0.75f) ? 1 : 0;
                f->cover = 0;
                f->tick += 1;
                MF_FRAME_BBOX_ADVANCE(f);
                if (a.adv.host_mirror) *a.adv.host_mirror = *f;
            } else {
                f->cover += cover;
            }
        }
    }
    if (pyr) {
        // levels 1 and 2 of the tile: thread t takes level-1 texel b = t % 4 of the tile's level-2 texel t / 4 (4 per row).  Every thread of the
        // workgroup makes the call -- the quad broadcasts need whole wavefronts -- and only those with a texel inside the image read and write
        const int W1 = v.W >> 1, H1 = v.H >> 1, W2 = v.W >> 2, H2 = v.H >> 2;
        const int q = (int)threadIdx.x >> 2, b = (int)threadIdx.x & 3, bx = b & 1, by = b >> 1, lx2 = q & 3, ly2 = q >> 2;
        const int x2 = (tx0 >> 2) + lx2, y2 = (ty0 >> 2) + ly2;
        const bool inside = live && ly2 < (bin.tileH >> 2) && x2 < W2 && y2 < H2;
        float Rm[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) Rm[q] = v.pose->R[q];
        const float3 tm = f3(v.pose->t[0], v.pose->t[1], v.pose->t[2]);
        MapPx m4[4];
        if (inside) {
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int l = (4 * ly2 + 2 * by + dy) * kTile + 4 * lx2 + 2 * bx + dx;
                    const float4 r = s_ray[l];
                    const unsigned long long w = s_key[l];
                    MapPx& m = m4[dy * 2 + dx];
                    m.v = f3(r.x, r.y, r.z); m.n = f3(r.w, __uint_as_float((unsigned)(w & 0xFFFFFFFFull)), __uint_as_float((unsigned)(w >> 32)));
                    m.vok = !isnan(m.v.x); m.nok = !isnan(m.n.x);
                }
        }
        model_pyramid_down(m4, inside, b, Rm, tm, a.vm[1], a.nm[1], W1 * H1, (2 * y2 + by) * W1 + 2 * x2 + bx, a.vm[2], a.nm[2], W2 * H2, y2 * W2 + x2);
    }
}

// GlobalProjection (Core/Model/GlobalProjection.cpp:43-114, splat_models.vert / combo_splat_models.frag) of ONE model through the
// same tile lists: the z-test winner of every pixel of the tile is merged into the key image with a plain read-modify-write --
// a pixel belongs to exactly one workgroup of this launch, and the other models' launches are ordered on the stream.  Same keys
// as k_global_scatter (mf_segment.hip), which stays for small (object) models: one global atomic per covered pixel is memory-side
// work (see the header) and cost ~170 us per frame for a 250 k-surfel background model against ~25 us here.
struct GlobalTileArgs { BinArgs b; unsigned payload; unsigned long long* keys; };
template <int kSpriteLanes>
__global__ __launch_bounds__(1024) void k_global_tile(const GlobalTileArgs a) {
    __shared__ unsigned long long s_key[kTile * kTileHMax];
    __shared__ float4 s_ray[kTile * kTileHMax];
    __shared__ int s_range[1];
    const BinArgs& bin = a.b;
    const int tile = xcd_contiguous_tile(blockIdx.x, bin.tilesX * bin.tilesY);
    if (tile >= bin.tilesX * bin.tilesY) return;
    TileStamps unused;
    tile_ztest<false, kSpriteLanes>(bin, tile, a.payload, s_key, s_ray, s_range, false, unused);
    const int px = (tile % bin.tilesX) * kTile + (threadIdx.x & (kTile - 1)), py = (tile / bin.tilesX) * bin.tileH + (threadIdx.x >> 4);
    if ((int)threadIdx.x >= kTile * bin.tileH || px >= bin.v.W || py >= bin.v.H) return;
    const unsigned long long key = s_key[threadIdx.x];
    if (key == kEmptyKey) return;
    const int p = py * bin.v.W + px;
    if (key < a.keys[p]) a.keys[p] = key;
}

size_t splat_tiles_scratch_ints(int W, int H) { return (size_t)((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile); }

// What both tiled passes start with: the arguments their two launches share, and the binning pass enqueued -- in a launch of its own, or
// (filter->fused, the prediction's rider) in the next frame's depth filter's
static BinArgs launch_bin(const SpriteView& v, const TileLists& l, const TileShape& t, const VisList* vis, const SplatFilterJob* filter, hipStream_t s) {
    const int nt = t.tilesX * t.tilesY;
    BinArgs b;
    b.v = v; b.tilesX = t.tilesX; b.tilesY = t.tilesY; b.tileH = t.tileH;
    b.tile_count = l.tile_count; b.entries = l.entries; b.tile_cap = l.entries_cap / nt;
    b.rec0 = l.rec0; b.rec1 = l.rec1; b.bbox = reinterpret_cast<short4*>(l.bbox);
    b.vis_list = vis ? vis->list : nullptr; b.vis_count = vis ? vis->count : nullptr;
    if (filter && filter->fused) {
        const int nbin = xcd_padded_grid(min(4 * 512, (v.src.cap + 2 * kBinFilterThreads - 1) / (2 * kBinFilterThreads))), nfil = bilateral_grid(v.W, v.H);
        const size_t lds = std::max((size_t)2 * nt * sizeof(int), (size_t)(kBLdsH * kBLdsW) * sizeof(float));
        // (eight 256-thread workgroups per compute unit: 2 048 are resident at once)
        hipLaunchKernelGGL(k_bin_bilateral, dim3(nbin + nfil), dim3(kBinFilterThreads), lds, s, b, nbin, (nbin + nfil > 2048) ? 1 : 0, filter->depth, filter->out, v.W, v.H);
        return b;
    }
    // two 1024-thread workgroups fit on a CU (60 VGPRs): 512 workgroups are ONE round of chunks up to a million surfels (with 256 a
    // 0.6 M-surfel map was 293 chunks = two rounds, the second one on 37 CUs)
    const int nblocks = min(512, (v.src.cap + 2 * kBinThreads - 1) / (2 * kBinThreads));
    hipLaunchKernelGGL(k_splat_bin, dim3(nblocks), dim3(kBinThreads), (size_t)2 * nt * sizeof(int), s, b);
    if (filter) launch_bilateral(filter->depth, filter->out, v.W, v.H, s);
    return b;
}
// the instance of a tile kernel K<lanes per sprite> ("spriteLanes": splat_sprite_lanes admits 1, 2, 4, 8, 16)
#define MF_LAUNCH_SPRITE_LANES(K, lanes, grid, threads, s, ...)                                              \
    switch (lanes) {                                                                                         \
        case 1: hipLaunchKernelGGL(K<1>, dim3(grid), dim3(threads), 0, s, __VA_ARGS__); break;               \
        case 2: hipLaunchKernelGGL(K<2>, dim3(grid), dim3(threads), 0, s, __VA_ARGS__); break;               \
        case 8: hipLaunchKernelGGL(K<8>, dim3(grid), dim3(threads), 0, s, __VA_ARGS__); break;               \
        case 16: hipLaunchKernelGGL(K<16>, dim3(grid), dim3(threads), 0, s, __VA_ARGS__); break;             \
        default: hipLaunchKernelGGL(K<4>, dim3(grid), dim3(threads), 0, s, __VA_ARGS__); break;              \
    }

int launch_global_tiled(const SpriteView& v, const TileLists& lists, unsigned payload, unsigned long long* keys, const VisList* vis, hipStream_t s) {
    const TileShape shape = splat_tile_shape(v.W, v.H, lists.tune);
    if (!shape.fits) return -1;
    const GlobalTileArgs t{launch_bin(v, lists, shape, vis, nullptr, s), payload, keys};
    MF_LAUNCH_SPRITE_LANES(k_global_tile, shape.lanes, xcd_padded_grid(shape.tilesX * shape.tilesY), shape.threads, s, t);
    return 0;
}

int launch_splat_tiled(const SpriteView& v, const TileLists& lists, const PredOut& out, const SplatRiders& riders, const VisList* vis, hipStream_t s) {
    const TileShape shape = splat_tile_shape(v.W, v.H, lists.tune);
    if (!shape.fits) return -1;
    TileArgs t;
    t.b = launch_bin(v, lists, shape, vis, riders.filter, s);
    t.out = out;
    t.prof = riders.prof;
    t.advance = riders.advance ? 1 : 0;
    t.adv = riders.advance ? *riders.advance : FrameAdvance{nullptr, nullptr, nullptr};
    t.tile_wgs = xcd_padded_grid(shape.tilesX * shape.tilesY);
    const SplatPyramidJob* pyramid = riders.pyramid;
    for (int i = 0; i < 3; ++i) { t.vm[i] = pyramid ? pyramid->vm[i] : nullptr; t.nm[i] = pyramid ? pyramid->nm[i] : nullptr; }
    FramePyrArgs fp{};
    int grid = t.tile_wgs;
    if (pyramid && pyramid->frame_depth) {   // the next frame's pyramid behind the tile workgroups: shape.threads / 256 of its tiles per workgroup
        fp.depth = pyramid->frame_depth; fp.W = v.W; fp.H = v.H; fp.k = v.k; fp.cutoff = pyramid->frame_cutoff;
        for (int i = 0; i < 3; ++i) { fp.vmap[i] = pyramid->frame_vmap[i]; fp.nmap[i] = pyramid->frame_nmap[i]; }
        const int nsub = shape.threads >> 8, groups = xcd_padded_grid(frame_pyramid_tiles(v.W, v.H)) >> 3;
        grid += ((groups + nsub - 1) / nsub) << 3;
    }
    MF_LAUNCH_SPRITE_LANES(k_splat_tile, shape.lanes, grid, shape.threads, s, t, fp);
    return 0;
}

}  // namespace mf
