// mf_mesh.hip -- a triangle mesh of a surfel cloud: naive surface nets over a moving-least-squares signed distance to the surfels' tangent
// planes (mf_cloud_mesh_build_dev / mf_cloud_mesh_emit_dev / mf_cloud_mesh_free; DESIGN.md "Surfel meshing").  No upstream twin: the
// reference writes its surfels (savePly) and never a surface.  The neighbourhoods are those of mf_eval.hip's cloud grid (mf_cloud_grid.h),
// built here by nn_build with cell edge h = support.
//
// The definition (include/maskfusion_amd.h has it in full).  A point is ELIGIBLE when its position and normal are finite and the normal is not
// zero; normals are normalised in fp64.  Lattice corner (i, j, k) stands at xf = (float)((double)origin + (double)i * (double)voxel) per axis.
// Its neighbours are the eligible points that pass mf_cloud_nn_dev's fp32 radius test against xf with radius `support` (d2 = dx*dx + dy*dy +
// dz*dz, no contraction, d2 <= fl(support * support)).  With d = xf - p in fp64 and q = (d . d) * (1 / support^2):  w = max(1 - q, 0)^2,
// W = sum w, f = sum w (n . d) / W, a = sum w n / W, c = sum w colour / W.  The corner is VALID with >= min_neighbours neighbours and W > 0,
// INSIDE when valid and f < 0.  Cell (i, j, k) -- corners (i + {0,1}, j + {0,1}, k + {0,1}) -- is ACTIVE when all eight are valid and not all
// on one side.  Lattice edge c -> c + e_a (u = (a + 1) mod 3, w = (a + 2) mod 3) with both ends valid and on different sides gives one quad
// when the cells c, c - e_u, c - e_u - e_w, c - e_w are all active: the vertices of those cells in that order when f(c) < 0, in the reverse
// order otherwise (counter-clockwise seen from f > 0).  A cell carries a vertex iff a quad names it: the mean over its sign-changing edges
// (x-edges first, then y, then z; within an axis the edges at (du, dw) = (0,0), (1,0), (0,1), (1,1)) of xa + t (xb - xa), t = fa / (fa - fb),
// in fp64 from the fp32 corner positions; the normal is the normalised mean of a_a + t (a_b - a_a) (zero when that mean is zero), the colour
// the mean of c_a + t (c_b - c_a); all stored as fp32.
//
// Reproducibility.  The ORDER of vertices and quads is a function of the inputs alone: every index comes from an ordered integer scan (blocks
// in directory order, corners in block order, the three axes of a corner in order), never from an atomic's rank.  The fp64 sums of a corner
// follow the grid's bucket order, which is the order of the build's atomics: f, a, c and with them positions, normals and colours are
// reproducible to rounding only, like the normals of mf_cloud_normals_dev.  (A corner whose f lies within that rounding of zero could change
// side between two calls; the tests assert that their fixtures have none.)
//
// Shape.  Memory and work follow the occupied part of the lattice.  The lattice is cut into blocks of 8 x 8 x 8 corners; a dense directory
// holds one unsigned per block (4 B per 512 corners: the only thing that grows with the volume, and the reason for the directory limit).
//   1. k_mesh_prep: one lane per point: the eligible points as float4 (the others NaN, which the grid does not hold), the unit normals as
//      [n][4] doubles, and a plain store of 1 into the directory entry of every block that holds a corner the point can be a neighbour of:
//      the corners within support of it per axis, widened by one corner on each side for the roundings (the point's reach of
//      ceil(support / voxel) + 1 cells).  Idempotent stores, no atomic.
//   2. nn_build (mf_eval.hip) of the float4 copy; nn_exclusive_scan of the directory: entry b becomes the block's slot, and b is occupied
//      iff dir[b + 1] > dir[b].  k_mesh_list writes the occupied blocks' ids by slot.  Corner (i, j, k) lives at slot * 512 + its place
//      in the block; a corner of a block that is not occupied has no neighbour and is not valid (mesh_slot returns -1).
//   3. k_mesh_field, the hot path: one wavefront per 4 x 4 x 4 corner tile (8 tiles a block).  The 64 lanes walk the union of their cell
//      ranges in step: nn_cell_range of the tile's lowest and highest coordinate (the bounds are monotone in x, so these enclose every
//      lane's own range), a cell skipped when its box lies beyond the radius of the whole tile (mesh_box_gap: nn_box_gap's widened box
//      against the interval, a lower bound of every lane's gap).  Every lane then tests the same record: the tile index is made uniform
//      with readfirstlane, so the loop control is scalar and bucket bounds, records, normals and colours are loads of one address per
//      wavefront (from scalar base registers).  A record counts only in the visit of its OWN
//      cell (nn_walk_records' rule for sums), and each lane applies the fp32 radius test itself: a lane's neighbours are exactly those
//      nn_walk_records would hand it.  Eight fp64 accumulators and a count per lane; no LDS, no atomics.
//   4. k_mesh_classify (one lane per cell), k_mesh_quads (one lane per corner: its three edges; flags the quad and, by plain stores, the
//      four cells it names), nn_exclusive_scan of both flag arrays, and on mf_cloud_mesh_emit_dev k_mesh_emit_vertices / k_mesh_emit_quads.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/maskfusion_amd.h"
#include "mf_internal.h"
#include "mf_device.h"
#include "mf_cloud_grid.h"

namespace mf {

constexpr int kMeshBlockCorners = 512;                  // 8 x 8 x 8
constexpr int64_t kMeshMaxDirectory = (int64_t)1 << 27; // blocks the directory indexes (512 MiB of entries)
constexpr int64_t kMeshMaxBlocks = 1 << 20;             // occupied blocks: 3 * 512 quad flags a block stay below 2^31
constexpr int kMeshFields = 7;                          // f, a (3), c (3)

struct MeshLattice {
    float origin[3], voxel, support;
    int dims[3], nb[3];      // corners and blocks per axis
    int min_nb;
    double inv_s2;           // 1 / support^2, fp64
};
struct MeshDev {
    MeshLattice L;
    const float* cloud; int stride, noff, coff, n;
    float4* pts;             // [n] the eligible points, NaN for the others
    double* nrm;             // [n][4] unit normals
    unsigned* dir;           // [ndir + 1] block -> slot (after the scan)
    unsigned* list;          // [nblk] slot -> block
    unsigned nblk, nslot;    // nslot = nblk * 512
    double* field;           // [kMeshFields][nslot]: f, ax, ay, az, cr, cg, cb (the colour planes only with coff >= 0)
    unsigned char* valid;    // [nslot] corners
    unsigned char* active;   // [nslot] cells, by the slot of their lowest corner
    unsigned* vscan;         // [nslot + 1] cells named by a quad: flags, then their exclusive scan
    unsigned* qscan;         // [3 nslot + 1] quads by (corner, axis): flags, then their exclusive scan
};

__device__ __forceinline__ float mesh_corner(const MeshLattice& L, int a, int i) {
    return (float)((double)L.origin[a] + (double)i * (double)L.voxel);
}
// the blocks along axis a that hold a corner x can be a neighbour of; false: none
__device__ __forceinline__ bool mesh_block_span(const MeshLattice& L, int a, float x, int& b0, int& b1) {
    const double o = (double)L.origin[a], v = (double)L.voxel, s = (double)L.support, top = (double)(L.dims[a] - 1);
    double lo = floor((((double)x - s) - o) / v) - 1.0, hi = ceil((((double)x + s) - o) / v) + 1.0;
    if (hi < 0.0 || lo > top) return false;
    lo = lo < 0.0 ? 0.0 : lo;
    hi = hi > top ? top : hi;
    b0 = (int)lo >> 3; b1 = (int)hi >> 3;
    return true;
}
__device__ __forceinline__ int mesh_local(int i, int j, int k) { return ((k & 7) * 8 + (j & 7)) * 8 + (i & 7); }
// the slot of corner (i, j, k); -1: outside the lattice, or in a block no point reaches
__device__ __forceinline__ int mesh_slot(const MeshDev& m, int i, int j, int k) {
    if (i < 0 || j < 0 || k < 0 || i >= m.L.dims[0] || j >= m.L.dims[1] || k >= m.L.dims[2]) return -1;
    const unsigned b = ((unsigned)(k >> 3) * m.L.nb[1] + (unsigned)(j >> 3)) * m.L.nb[0] + (unsigned)(i >> 3);
    const unsigned s0 = m.dir[b];
    if (m.dir[b + 1] == s0) return -1;
    return (int)(s0 * kMeshBlockCorners) + mesh_local(i, j, k);
}
// slot -> corner
__device__ __forceinline__ void mesh_corner_of(const MeshDev& m, unsigned s, int& i, int& j, int& k) {
    const unsigned b = m.list[s >> 9], l = s & 511u;
    const unsigned bx = b % (unsigned)m.L.nb[0], by = (b / (unsigned)m.L.nb[0]) % (unsigned)m.L.nb[1], bz = b / ((unsigned)m.L.nb[0] * (unsigned)m.L.nb[1]);
    i = (int)(bx * 8 + (l & 7u)); j = (int)(by * 8 + ((l >> 3) & 7u)); k = (int)(bz * 8 + (l >> 6));
}

// 1.
__global__ __launch_bounds__(kNnThreads) void k_mesh_prep(MeshDev m) {
    for (int i = blockIdx.x * kNnThreads + threadIdx.x; i < m.n; i += gridDim.x * kNnThreads) {
        const float* p = m.cloud + (size_t)i * m.stride;
        const float x = p[0], y = p[1], z = p[2], nx = p[m.noff], ny = p[m.noff + 1], nz = p[m.noff + 2];
        double ux = 0.0, uy = 0.0, uz = 0.0;
        bool ok = false;
        if (nn_finite(x, y, z) && nn_finite(nx, ny, nz)) {
            const double len = sqrt(((double)nx * (double)nx + (double)ny * (double)ny) + (double)nz * (double)nz);
            if (len > 0.0) { ok = true; ux = (double)nx / len; uy = (double)ny / len; uz = (double)nz / len; }
        }
        m.pts[i] = ok ? make_float4(x, y, z, 0.f) : make_float4(NAN, NAN, NAN, 0.f);
        double* o = m.nrm + (size_t)i * 4;
        o[0] = ux; o[1] = uy; o[2] = uz; o[3] = 0.0;
        int x0, x1, y0, y1, z0, z1;
        if (!ok || !mesh_block_span(m.L, 0, x, x0, x1) || !mesh_block_span(m.L, 1, y, y0, y1) || !mesh_block_span(m.L, 2, z, z0, z1)) continue;
        for (int bz = z0; bz <= z1; ++bz)
            for (int by = y0; by <= y1; ++by)
                for (int bx = x0; bx <= x1; ++bx) m.dir[((size_t)bz * m.L.nb[1] + by) * m.L.nb[0] + bx] = 1u;
    }
}
// 2.
__global__ __launch_bounds__(kNnThreads) void k_mesh_list(MeshDev m, unsigned ndir) {
    for (unsigned b = blockIdx.x * kNnThreads + threadIdx.x; b < ndir; b += gridDim.x * kNnThreads) {
        const unsigned s = m.dir[b];
        if (m.dir[b + 1] > s) m.list[s] = b;
    }
}

// 3.  squared distance from the interval [xlo, xhi] to cell c's widened box: no more than nn_box_gap(x, c) of any x in the interval
__device__ __forceinline__ double mesh_box_gap(const NnGrid& g, double xlo, double xhi, int c) {
    const double pad = g.h * 9.5367431640625e-07;
    const double lo = (double)c * g.h - pad, hi = (double)(c + 1) * g.h + pad;
    const double d = xhi < lo ? lo - xhi : (xlo > hi ? xlo - hi : 0.0);
    return d * d;
}
constexpr int kMeshWaves = kNnThreads / 64;   // tiles per workgroup
__global__ __launch_bounds__(kNnThreads) void k_mesh_field(NnGrid g, MeshDev m) {
    const int lane = threadIdx.x & 63;
    const unsigned ntile = m.nblk * 8u;
    for (unsigned t0 = blockIdx.x * kMeshWaves; t0 < ntile; t0 += gridDim.x * kMeshWaves) {
        if (t0 + (threadIdx.x >> 6) >= ntile) continue;
        const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)(t0 + (threadIdx.x >> 6)));   // the wavefront's tile, uniform
        const unsigned slot = t >> 3, b = m.list[slot];
        const unsigned bx = b % (unsigned)m.L.nb[0], by = (b / (unsigned)m.L.nb[0]) % (unsigned)m.L.nb[1], bz = b / ((unsigned)m.L.nb[0] * (unsigned)m.L.nb[1]);
        const int i0 = (int)(bx * 8 + (t & 1u) * 4), j0 = (int)(by * 8 + ((t >> 1) & 1u) * 4), k0 = (int)(bz * 8 + ((t >> 2) & 1u) * 4);
        if (i0 >= m.L.dims[0] || j0 >= m.L.dims[1] || k0 >= m.L.dims[2]) continue;   // a tile beyond the lattice (valid stays 0)
        const int i = i0 + (lane & 3), j = j0 + ((lane >> 2) & 3), k = k0 + (lane >> 4);
        const bool inside = i < m.L.dims[0] && j < m.L.dims[1] && k < m.L.dims[2];
        const float x = mesh_corner(m.L, 0, i), y = mesh_corner(m.L, 1, j), z = mesh_corner(m.L, 2, k);
        // the tile's extent, and the cells that enclose every lane's range
        const float xlo = mesh_corner(m.L, 0, i0), xhi = mesh_corner(m.L, 0, min(i0 + 3, m.L.dims[0] - 1));
        const float ylo = mesh_corner(m.L, 1, j0), yhi = mesh_corner(m.L, 1, min(j0 + 3, m.L.dims[1] - 1));
        const float zlo = mesh_corner(m.L, 2, k0), zhi = mesh_corner(m.L, 2, min(k0 + 3, m.L.dims[2] - 1));
        int x0, x1, y0, y1, z0, z1, unused;
        nn_cell_range(g, xlo, x0, unused); nn_cell_range(g, xhi, unused, x1);
        nn_cell_range(g, ylo, y0, unused); nn_cell_range(g, yhi, unused, y1);
        nn_cell_range(g, zlo, z0, unused); nn_cell_range(g, zhi, unused, z1);
        double W = 0.0, F = 0.0, ax = 0.0, ay = 0.0, az = 0.0, cr = 0.0, cg = 0.0, cb = 0.0;
        int cnt = 0;
        for (int cz = z0; cz <= z1; ++cz) {
            const double gz = mesh_box_gap(g, zlo, zhi, cz);
            for (int cy = y0; cy <= y1; ++cy) {
                const double gy = mesh_box_gap(g, ylo, yhi, cy);
                for (int cx = x0; cx <= x1; ++cx) {
                    const double gap = (gz + gy + mesh_box_gap(g, xlo, xhi, cx)) * (1.0 - 3.814697265625e-06);
                    if (gap > (double)g.r2) continue;
                    const unsigned bk = nn_hash(cx, cy, cz) & g.mask;
                    const unsigned e = g.start[bk + 1];
                    for (unsigned r = g.start[bk]; r < e; ++r) {
                        const float4 p = g.rec[r];
                        if (nn_cell(g, p.x) != cx || nn_cell(g, p.y) != cy || nn_cell(g, p.z) != cz) continue;   // another cell's record in a shared bucket
                        const float fx = p.x - x, fy = p.y - y, fz = p.z - z;
                        const float d2 = fx * fx + fy * fy + fz * fz;
                        if (!(d2 <= g.r2)) continue;
                        const int jp = __float_as_int(p.w);
                        const double* nj = m.nrm + (size_t)jp * 4;
                        const double nx = nj[0], ny = nj[1], nz = nj[2];
                        const double dx = (double)x - (double)p.x, dy = (double)y - (double)p.y, dz = (double)z - (double)p.z;
                        const double q = ((dx * dx + dy * dy) + dz * dz) * m.L.inv_s2;
                        double w = 1.0 - q;
                        w = w > 0.0 ? w : 0.0;
                        w = w * w;
                        W += w;
                        F += w * ((nx * dx + ny * dy) + nz * dz);
                        ax += w * nx; ay += w * ny; az += w * nz;
                        if (m.coff >= 0) {
                            const float* cp = m.cloud + (size_t)jp * m.stride + m.coff;
                            cr += w * (double)cp[0]; cg += w * (double)cp[1]; cb += w * (double)cp[2];
                        }
                        ++cnt;
                    }
                }
            }
        }
        if (!inside) continue;
        const size_t s = (size_t)slot * kMeshBlockCorners + mesh_local(i, j, k), ns = m.nslot;
        const bool ok = cnt >= m.L.min_nb && W > 0.0;
        m.valid[s] = ok ? 1 : 0;
        m.field[s] = ok ? F / W : 0.0;
        m.field[ns + s] = ok ? ax / W : 0.0; m.field[2 * ns + s] = ok ? ay / W : 0.0; m.field[3 * ns + s] = ok ? az / W : 0.0;
        if (m.coff >= 0) { m.field[4 * ns + s] = ok ? cr / W : 0.0; m.field[5 * ns + s] = ok ? cg / W : 0.0; m.field[6 * ns + s] = ok ? cb / W : 0.0; }
    }
}

// 4.  cells
__global__ __launch_bounds__(kNnThreads) void k_mesh_classify(MeshDev m) {
    for (unsigned s = blockIdx.x * kNnThreads + threadIdx.x; s < m.nslot; s += gridDim.x * kNnThreads) {
        int i, j, k;
        mesh_corner_of(m, s, i, j, k);
        int in = 0;
        bool all = true;
        for (int c = 0; c < 8 && all; ++c) {
            const int cs = mesh_slot(m, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2));
            if (cs < 0 || !m.valid[cs]) all = false;
            else in += m.field[cs] < 0.0 ? 1 : 0;
        }
        m.active[s] = (all && in > 0 && in < 8) ? 1 : 0;
    }
}
// the four cells around the edge from corner (i, j, k) along axis a, in the quad's order; false: one of them is not active
__device__ __forceinline__ bool mesh_quad_cells(const MeshDev& m, int i, int j, int k, int a, int (&cell)[4]) {
    const int u = (a + 1) % 3, w = (a + 2) % 3;
    const int du[4] = {0, -1, -1, 0}, dw[4] = {0, 0, -1, -1};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int c[3] = {i, j, k};
        c[u] += du[q]; c[w] += dw[q];
        cell[q] = mesh_slot(m, c[0], c[1], c[2]);
        if (cell[q] < 0 || !m.active[cell[q]]) return false;
    }
    return true;
}
__global__ __launch_bounds__(kNnThreads) void k_mesh_quads(MeshDev m) {
    for (unsigned s = blockIdx.x * kNnThreads + threadIdx.x; s < m.nslot; s += gridDim.x * kNnThreads) {
        if (!m.valid[s]) continue;
        int i, j, k;
        mesh_corner_of(m, s, i, j, k);
        const bool in = m.field[s] < 0.0;
        for (int a = 0; a < 3; ++a) {
            const int s2 = mesh_slot(m, i + (a == 0), j + (a == 1), k + (a == 2));
            if (s2 < 0 || !m.valid[s2] || (m.field[s2] < 0.0) == in) continue;
            int cell[4];
            if (!mesh_quad_cells(m, i, j, k, a, cell)) continue;
            m.qscan[3 * (size_t)s + a] = 1u;
            for (int q = 0; q < 4; ++q) m.vscan[cell[q]] = 1u;
        }
    }
}

// emit
struct MeshOut { float* v; float* nrm; float* col; int* cell; int* quad; };
__global__ __launch_bounds__(kNnThreads) void k_mesh_emit_vertices(MeshDev m, MeshOut o) {
    const size_t ns = m.nslot;
    for (unsigned s = blockIdx.x * kNnThreads + threadIdx.x; s < m.nslot; s += gridDim.x * kNnThreads) {
        const unsigned v = m.vscan[s];
        if (m.vscan[s + 1] == v) continue;
        int c0[3];
        mesh_corner_of(m, s, c0[0], c0[1], c0[2]);
        int cs[8];
        double f[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            cs[c] = mesh_slot(m, c0[0] + (c & 1), c0[1] + ((c >> 1) & 1), c0[2] + (c >> 2));
            f[c] = m.field[cs[c]];
        }
        double P[3] = {0.0, 0.0, 0.0}, A[3] = {0.0, 0.0, 0.0}, C[3] = {0.0, 0.0, 0.0};
        int cnt = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int u = (a + 1) % 3, w = (a + 2) % 3;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ca = ((e & 1) << u) | ((e >> 1) << w), cb = ca | (1 << a);
                const double fa = f[ca], fb = f[cb];
                if ((fa < 0.0) == (fb < 0.0)) continue;
                const double t = fa / (fa - fb);
                for (int d = 0; d < 3; ++d) {
                    const double xa = (double)mesh_corner(m.L, d, c0[d] + ((ca >> d) & 1)), xb = (double)mesh_corner(m.L, d, c0[d] + ((cb >> d) & 1));
                    P[d] += xa + t * (xb - xa);
                    const double aa = m.field[(1 + d) * ns + cs[ca]], ab = m.field[(1 + d) * ns + cs[cb]];
                    A[d] += aa + t * (ab - aa);
                    if (m.coff >= 0) {
                        const double ka = m.field[(4 + d) * ns + cs[ca]], kb = m.field[(4 + d) * ns + cs[cb]];
                        C[d] += ka + t * (kb - ka);
                    }
                }
                ++cnt;
            }
        }
        const double n = (double)cnt;
        for (int d = 0; d < 3; ++d) { P[d] = P[d] / n; A[d] = A[d] / n; C[d] = C[d] / n; }
        const double len = sqrt((A[0] * A[0] + A[1] * A[1]) + A[2] * A[2]);
        for (int d = 0; d < 3; ++d) {
            o.v[(size_t)v * 3 + d] = (float)P[d];
            if (o.nrm) o.nrm[(size_t)v * 3 + d] = len > 0.0 ? (float)(A[d] / len) : 0.f;
            if (o.col) o.col[(size_t)v * 3 + d] = (float)C[d];
            if (o.cell) o.cell[(size_t)v * 3 + d] = c0[d];
        }
    }
}
__global__ __launch_bounds__(kNnThreads) void k_mesh_emit_quads(MeshDev m, MeshOut o) {
    const size_t nq3 = (size_t)m.nslot * 3;
    for (size_t e = (size_t)blockIdx.x * kNnThreads + threadIdx.x; e < nq3; e += (size_t)gridDim.x * kNnThreads) {
        const unsigned q = m.qscan[e];
        if (m.qscan[e + 1] == q) continue;
        const unsigned s = (unsigned)(e / 3);
        const int a = (int)(e - (size_t)s * 3);
        int i, j, k, cell[4];
        mesh_corner_of(m, s, i, j, k);
        mesh_quad_cells(m, i, j, k, a, cell);
        const bool in = m.field[s] < 0.0;
        for (int c = 0; c < 4; ++c) o.quad[(size_t)q * 4 + c] = (int)m.vscan[cell[in ? c : 3 - c]];
    }
}

// ---------------- host side ----------------
static thread_local std::string t_cloud_error;     // the reason of the last failure of a call that has no context (mf_last_error(NULL))
const char* cloud_last_error() { return t_cloud_error.empty() ? nullptr : t_cloud_error.c_str(); }
int cloud_fail(const char* who, const char* text, int rc) {
    t_cloud_error = std::string(who) + text;
    return rc;
}
static int mesh_fail(const char* text, int rc) { return cloud_fail("mf_cloud_mesh: ", text, rc); }

}  // namespace mf

using namespace mf;

struct mf_mesh {
    MeshDev m;
    uint32_t nv = 0, nq = 0;
    void* d_dir = nullptr; void* d_blocks = nullptr;     // the directory; everything sized by the occupied blocks, one allocation
};

static int mesh_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kNnThreads - 1) / kNnThreads, kNnMaxGrid)); }
static uint64_t mesh_align(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

// the checks that need no device; on success L is filled
static int mesh_check(const float* d_points, int32_t stride, int32_t normal_offset, int32_t color_offset, int64_t n, const float* origin3, float voxel,
                      const int32_t* dims3, float support, int32_t min_neighbours, mf_mesh** out, uint32_t* n_vertices, uint32_t* n_quads, MeshLattice& L) {
    if (!out || !n_vertices || !n_quads || !origin3 || !dims3) return mesh_fail("null pointer", MF_EINVAL);
    if (n < 0 || n > (int64_t)1 << 30) return mesh_fail("point count out of range (0 .. 2^30)", MF_EINVAL);
    if (n > 0 && !d_points) return mesh_fail("null points", MF_EINVAL);
    if (stride < 6 || normal_offset < 3 || normal_offset + 3 > stride) return mesh_fail("stride must be >= 6 floats and the normal lie at 3 .. stride - 3", MF_EINVAL);
    if (color_offset >= 0 && (color_offset < 3 || color_offset + 3 > stride)) return mesh_fail("the colour must lie at 3 .. stride - 3 (or offset < 0: none)", MF_EINVAL);
    if (!(std::isfinite(voxel) && voxel > 0.f)) return mesh_fail("voxel must be finite and > 0", MF_EINVAL);
    if (!(std::isfinite(support) && support >= voxel && support <= 8.f * voxel)) return mesh_fail("support must lie in voxel .. 8 voxel", MF_EINVAL);
    if (min_neighbours < 1) return mesh_fail("min_neighbours must be >= 1", MF_EINVAL);
    int64_t ndir = 1;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin3[a])) return mesh_fail("origin is not finite", MF_EINVAL);
        if (dims3[a] < 2) return mesh_fail("dims must be >= 2 corners per axis", MF_EINVAL);
        const double top = (double)origin3[a] + (double)(dims3[a] - 1) * (double)voxel;
        if (!(std::fabs((double)origin3[a]) / (double)support < kNnCellLimit - 2.0 && std::fabs(top) / (double)support < kNnCellLimit - 2.0))
            return mesh_fail("a lattice corner has |x / support| >= 2^30", MF_EINVAL);
        L.origin[a] = origin3[a]; L.dims[a] = dims3[a]; L.nb[a] = (dims3[a] + 7) / 8;
        ndir *= L.nb[a];
        if (ndir > kMeshMaxDirectory) return mesh_fail("the lattice has more than 2^27 blocks of 8 x 8 x 8 corners", MF_EINVAL);
    }
    L.voxel = voxel; L.support = support; L.min_nb = min_neighbours;
    L.inv_s2 = 1.0 / ((double)support * (double)support);
    return MF_OK;
}

extern "C" void mf_cloud_mesh_free(mf_mesh* h) {
    if (!h) return;
    if (h->d_dir) (void)hipFree(h->d_dir);
    if (h->d_blocks) (void)hipFree(h->d_blocks);
    delete h;
}

extern "C" int mf_cloud_mesh_build_dev(const float* d_points, int32_t stride, int32_t normal_offset, int32_t color_offset, int64_t n, const float* origin3,
                                       float voxel, const int32_t* dims3, float support, int32_t min_neighbours, mf_mesh** out, uint32_t* n_vertices,
                                       uint32_t* n_quads, float* stage_ms, void* stream) {
    MeshLattice L;
    memset(&L, 0, sizeof(L));
    int rc = mesh_check(d_points, stride, normal_offset, color_offset, n, origin3, voxel, dims3, support, min_neighbours, out, n_vertices, n_quads, L);
    if (rc != MF_OK) return rc;
    *out = nullptr; *n_vertices = 0; *n_quads = 0;
    if (stage_ms) for (int k = 0; k < MF_MESH_STAGES; ++k) stage_ms[k] = 0.f;
    mf_mesh* h = new mf_mesh();
    memset(&h->m, 0, sizeof(h->m));
    h->m.L = L; h->m.coff = color_offset;
    if (n == 0) { *out = h; return MF_OK; }

    hipStream_t s = (hipStream_t)stream;
    MeshDev& m = h->m;
    m.cloud = d_points; m.stride = stride; m.noff = normal_offset; m.n = (int)n;
    const uint64_t ndir = (uint64_t)L.nb[0] * L.nb[1] * L.nb[2];
    void* d_tmp = nullptr;                  // points | normals | the grid's workspace: freed when the field is done
    hipEvent_t ev[MF_MESH_STAGES + 1];
    int n_ev = 0;
    auto stamp = [&] { if (stage_ms && n_ev <= MF_MESH_STAGES) (void)hipEventRecord(ev[n_ev++], s); };
    auto done = [&](int code, const char* text) {
        if (d_tmp) (void)hipFree(d_tmp);
        if (stage_ms) for (int k = 0; k <= MF_MESH_STAGES; ++k) (void)hipEventDestroy(ev[k]);
        if (code != MF_OK) { mf_cloud_mesh_free(h); return mesh_fail(text, code); }
        *out = h; *n_vertices = h->nv; *n_quads = h->nq;
        return (int)MF_OK;
    };
    if (stage_ms) for (int k = 0; k <= MF_MESH_STAGES; ++k) if (hipEventCreate(&ev[k]) != hipSuccess) { stage_ms = nullptr; break; }

    // directory [ndir + 1] | scan sums
    const uint64_t dir_bytes = mesh_align((ndir + 1) * 4);
    if (hipMalloc(&h->d_dir, dir_bytes + mesh_align(kNnScanBlocks * 4)) != hipSuccess) return done(MF_ENOMEM, "hipMalloc of the block directory failed");
    m.dir = (unsigned*)h->d_dir;
    unsigned* sums = (unsigned*)((char*)h->d_dir + dir_bytes);
    const uint64_t pts_bytes = mesh_align((uint64_t)n * 16), nrm_bytes = mesh_align((uint64_t)n * 32);
    if (hipMalloc(&d_tmp, pts_bytes + nrm_bytes + nn_workspace_bytes(n)) != hipSuccess) return done(MF_ENOMEM, "hipMalloc of the grid failed");
    m.pts = (float4*)d_tmp;
    m.nrm = (double*)((char*)d_tmp + pts_bytes);
    const NnGrid g = nn_layout((char*)d_tmp + pts_bytes + nrm_bytes, n, support);

    stamp();
    if (hipMemsetAsync(m.dir, 0, (ndir + 1) * 4, s) != hipSuccess) return done(MF_EHIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(k_mesh_prep, dim3(mesh_blocks(n)), dim3(kNnThreads), 0, s, m);
    nn_exclusive_scan(m.dir, sums, (unsigned)ndir, s);
    stamp();
    const char* why = nullptr;
    rc = nn_build(g, (const float*)m.pts, 4, -1, nullptr, n, s, &why);
    if (rc != MF_OK) return done(rc, why ? why : "the grid build failed");
    stamp();                                // (the next stage is the host's: the wait, the block count read back, the allocation)
    rc = nn_finish(g, s, &why);
    if (rc != MF_OK) return done(rc, rc == MF_EINVAL ? "an eligible point has |x / support| >= 2^30" : (why ? why : "HIP error"));
    unsigned nblk = 0;
    if (hipMemcpy(&nblk, m.dir + ndir, 4, hipMemcpyDeviceToHost) != hipSuccess) return done(MF_EHIP, "hipMemcpy failed");
    if (nblk == 0) return done(MF_OK, nullptr);
    if ((int64_t)nblk > kMeshMaxBlocks) return done(MF_ENOMEM, "more than 2^20 occupied blocks: mesh a part of the lattice, or use a larger voxel");

    // everything by slot: list | field | valid | active | vscan | qscan
    const uint64_t ns = (uint64_t)nblk * kMeshBlockCorners;
    const int planes = color_offset >= 0 ? kMeshFields : 4;
    const uint64_t o_field = mesh_align((uint64_t)nblk * 4), o_valid = o_field + mesh_align(ns * 8 * planes), o_active = o_valid + mesh_align(ns),
                   o_vscan = o_active + mesh_align(ns), o_qscan = o_vscan + mesh_align((ns + 1) * 4), total = o_qscan + mesh_align((3 * ns + 1) * 4);
    if (hipMalloc(&h->d_blocks, total) != hipSuccess) return done(MF_ENOMEM, "hipMalloc of the occupied blocks failed");
    char* w = (char*)h->d_blocks;
    m.nblk = nblk; m.nslot = (unsigned)ns;
    m.list = (unsigned*)w; m.field = (double*)(w + o_field); m.valid = (unsigned char*)(w + o_valid); m.active = (unsigned char*)(w + o_active);
    m.vscan = (unsigned*)(w + o_vscan); m.qscan = (unsigned*)(w + o_qscan);
    stamp();
    if (hipMemsetAsync(w + o_valid, 0, total - o_valid, s) != hipSuccess) return done(MF_EHIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(k_mesh_list, dim3(mesh_blocks((int64_t)ndir)), dim3(kNnThreads), 0, s, m, (unsigned)ndir);
    hipLaunchKernelGGL(k_mesh_field, dim3((unsigned)std::min<uint64_t>(((uint64_t)nblk * 8 + kMeshWaves - 1) / kMeshWaves, kNnMaxGrid)), dim3(kNnThreads), 0, s, g, m);
    stamp();
    hipLaunchKernelGGL(k_mesh_classify, dim3(mesh_blocks((int64_t)ns)), dim3(kNnThreads), 0, s, m);
    hipLaunchKernelGGL(k_mesh_quads, dim3(mesh_blocks((int64_t)ns)), dim3(kNnThreads), 0, s, m);
    stamp();
    nn_exclusive_scan(m.vscan, sums, (unsigned)ns, s);
    nn_exclusive_scan(m.qscan, sums, (unsigned)(3 * ns), s);
    stamp();
    if (hipGetLastError() != hipSuccess) return done(MF_EHIP, "kernel launch failed");
    if (hipMemcpyAsync(&h->nv, m.vscan + ns, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&h->nq, m.qscan + 3 * ns, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return done(MF_EHIP, "HIP error during the meshing kernels");
    if (stage_ms && n_ev == MF_MESH_STAGES + 1)
        for (int k = 0; k < MF_MESH_STAGES; ++k) (void)hipEventElapsedTime(&stage_ms[k], ev[k], ev[k + 1]);
    // the handle keeps no pointer into the caller's cloud or the grid
    m.cloud = nullptr; m.pts = nullptr; m.nrm = nullptr;
    return done(MF_OK, nullptr);
}

extern "C" int mf_cloud_mesh_emit_dev(const mf_mesh* h, float* d_vertices, float* d_normals, float* d_colors, int32_t* d_cells, int32_t* d_quads,
                                      void* stream) {
    if (!h) return mesh_fail("null handle", MF_EINVAL);
    if ((h->nv > 0 && !d_vertices) || (h->nq > 0 && !d_quads)) return mesh_fail("null output", MF_EINVAL);
    if (d_colors && h->m.coff < 0) return mesh_fail("colours asked of a mesh built without them", MF_EINVAL);
    if (h->nv == 0) return MF_OK;
    hipStream_t s = (hipStream_t)stream;
    MeshOut o = {d_vertices, d_normals, d_colors, d_cells, d_quads};
    hipLaunchKernelGGL(k_mesh_emit_vertices, dim3(mesh_blocks((int64_t)h->m.nslot)), dim3(kNnThreads), 0, s, h->m, o);
    if (h->nq > 0) hipLaunchKernelGGL(k_mesh_emit_quads, dim3(mesh_blocks(3 * (int64_t)h->m.nslot)), dim3(kNnThreads), 0, s, h->m, o);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return mesh_fail("HIP error during the emit kernels", MF_EHIP);
    return MF_OK;
}
