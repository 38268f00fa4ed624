// mf_trimesh_ray.hip -- ray casting against a triangle mesh: for every ray the first triangle it hits, over the cell grid and the wide list
// that mf_trimesh_build_dev made (mf_trimesh_raycast_dev / mf_trimesh_render_dev; DESIGN.md "Mesh rendering").  No upstream twin: the
// reference never renders a mesh.
//
// The definition (include/maskfusion_amd.h has it in full).  The ray is mapped by the fp32 transform; then everything is fp64 from the fp32
// values, every operation rounded on its own (the file is compiled without contraction): the watertight test of Woop, Benthin and Wald
// (JCGT 2013) -- the ray's dominant axis kz, the shear Sx, Sy, Sz, the sheared vertices, the edge functions U, V, W, det = (U + V) + W,
// t = ((U Az + V Bz) + W Cz) / det.  A triangle COUNTS when its edge functions do not differ in sign, det != 0 and tmin <= t <= tmax; the
// result is the minimum over (t, index) of the counting eligible triangles: a function of the mesh and the ray alone, whatever the cell
// and whichever structure found the triangle.
//
// Shape.
//   0. k_tri_bounds (at the end of the build): the fp32 bounding box of the GRIDDED triangles (eligible, not wide), as six order-preserving
//      integer keys under atomicMax -- a maximum's value does not depend on the order of its atomics --, a wave folded by shuffles first.
//   1. k_tri_raycast, the hot path: one lane per ray; the pinhole form gives the 64 lanes of a wavefront an 8 x 8 pixel tile, so that they
//      walk the same cells and load the same buckets.  ray_cast is the one device function of both forms.
//      The walk is parametrised by z, the coordinate along the ray's dominant axis kz: x(z) = o[kx] + Sx (z - o[kz]) with |Sx|, |Sy| <= 1.
//      The ray is clipped to the box widened by one cell and to [tmin, tmax]: an interval [z0, z1] of z.  The layers of cells along kz that
//      [z0, z1] touches are visited in the ray's direction; in a layer, every cell that the ray's extent on kx and ky over the layer's
//      slab touches, each extent widened by `pad`, the cells clamped to the box's.  The walk stops at the first layer whose entry
//      parameter, less 2 pad / |d[kz]|, lies beyond the best t so far.  Then the wide list, every triangle of it, one skipped only when the
//      ray's piece over the triangle's z-range, widened by pad, misses the triangle's box or lies beyond [tmin, min(tmax, best t)].
//      A triangle met twice (several cells hold it; two cells share a bucket) is harmless for a minimum over (t, index); the one already
//      best is skipped.
//
// No counting triangle can be skipped.  Write M = max |o| + max |box coordinate| and eps = 2^-53.
//   Where the computed hit lies.  A vertex's sheared Px, Py are computed once and serve both edges that share it, each within 4 eps M of
//   its exact value; the rounding of an edge function's two products and their difference is that of moving its end points by 2 eps more
//   of their size.  So when U, V, W do not differ in sign and det != 0, the sheared origin lies in a triangle whose corners are within
//   8 eps M of the exact sheared corners, and U / det, V / det, W / det are its barycentric weights there.  t is the same weights' mean of
//   Az, Bz, Cz to 4 eps, so H = o + t d (o, d, t as computed; H a real point) has H[kz] within 8 eps M of the hull of the corners' kz
//   coordinates, and, since the weighted sheared coordinates cancel to 8 eps M, H[kx] and H[ky] within 16 eps M = 2^-49 M of the hulls of
//   theirs: H lies in the triangle's bounding box widened by 2^-49 M.  Let H' be H moved into that box.
//   Its cell is listed.  nn_cell is monotone (one rounded product, one floor), so on each axis the cell of H' lies between the cells of
//   the box's fp32 ends, which are the cells the build listed the triangle in; and inside the cells of the box of all gridded triangles.
//   Its cell is visited.  pad = 2^-18 cell + 2^-44 M is 32 times the 2^-49 M above and more than 2^6 times any rounding of the walk's own
//   few operations on values of size M (z0, z1, a slab's ends against nn_cell's product, x(z)).  H[kz] satisfies the three clips up to
//   that rounding -- t is in [tmin, tmax]; a hit inside the box is a whole cell inside the widened box, which on a minor axis is at least a
//   cell of z, |S| being <= 1 -- so the layer of H'[kz] is within [floor(z0 / cell), floor(z1 / cell)] and its slab, widened by pad,
//   holds H[kz]; the ray's extent over that slab then holds H[kx], H[ky], and widened by pad it holds those of H'.
//   The early stop.  Every triangle whose H' lies in the layer at hand or a later one has t >= entry - pad / |d[kz]| - rounding >
//   entry - 2 pad / |d[kz]|.  The walk stops only when that bound is GREATER than the best t: such a triangle can neither win nor tie.  The
//   best t never falls below the final minimum, so the winner's layer is reached.
//   The wide list's slab test is the same statement for one triangle's own box.
// pad grows with |o|: a ray that starts 2^26 cells or more from the mesh visits a wide band of cells (it stays correct).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "mf_trimesh.h"

namespace mf {

constexpr int kRayTile = 8;                    // the pinhole form: a wavefront's lanes are an 8 x 8 tile of pixels
constexpr int kRayBoundsBlocks = 128;
constexpr int kRayMaxLayerCells = 32768;       // 2^15: the cells the gridded triangles may span on an axis
constexpr double kRayPadCell = 3.814697265625e-06;       // 2^-18 of a cell
constexpr double kRayPadSize = 5.684341886080802e-14;    // 2^-44 of M

// ---------------- 0. the box of the gridded triangles ----------------
// finite floats in their order as unsigned keys > 0; the minimum is kept as the maximum of the complement
__host__ __device__ __forceinline__ unsigned ray_key(float x) {
    unsigned b;
    memcpy(&b, &x, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float ray_unkey(unsigned k) {
    const unsigned b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float x;
    memcpy(&x, &b, 4);
    return x;
}
__global__ __launch_bounds__(kNnThreads) void k_tri_bounds(TriDev m, unsigned* keys) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = blockIdx.x * kNnThreads + threadIdx.x; t < m.nt; t += gridDim.x * kNnThreads) {
        const float4 a = m.rec[(size_t)t * 3], b = m.rec[(size_t)t * 3 + 1], c = m.rec[(size_t)t * 3 + 2];
        if (__float_as_int(a.w) < 0) continue;
        int clo[3], chi[3];
        if (tri_box_cells(m.g, a, b, c, clo, chi) < 0) continue;
        lo[0] = fminf(lo[0], fminf(a.x, fminf(b.x, c.x))); lo[1] = fminf(lo[1], fminf(a.y, fminf(b.y, c.y))); lo[2] = fminf(lo[2], fminf(a.z, fminf(b.z, c.z)));
        hi[0] = fmaxf(hi[0], fmaxf(a.x, fmaxf(b.x, c.x))); hi[1] = fmaxf(hi[1], fmaxf(a.y, fmaxf(b.y, c.y))); hi[2] = fmaxf(hi[2], fmaxf(a.z, fmaxf(b.z, c.z)));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        for (int s = 32; s >= 1; s >>= 1) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], s));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], s));
        }
    }
    if ((threadIdx.x & 63) == 0 && lo[0] <= hi[0]) {
        atomicMax(&keys[0], ~ray_key(lo[0])); atomicMax(&keys[1], ~ray_key(lo[1])); atomicMax(&keys[2], ~ray_key(lo[2]));
        atomicMax(&keys[3], ray_key(hi[0])); atomicMax(&keys[4], ray_key(hi[1])); atomicMax(&keys[5], ray_key(hi[2]));
    }
}
void tri_bounds_dev(const TriDev& m, hipStream_t s) {
    hipLaunchKernelGGL(k_tri_bounds, dim3(tri_blocks(m.nt, kRayBoundsBlocks)), dim3(kNnThreads), 0, s, m, (unsigned*)((char*)m.counters + kTriBoundsAt));
}
bool tri_bounds_read(const unsigned* keys6, float* lo3, float* hi3) {
    if (!keys6[0]) return false;
    for (int k = 0; k < 3; ++k) { lo3[k] = ray_unkey(~keys6[k]); hi3[k] = ray_unkey(keys6[3 + k]); }
    return true;
}

// ---------------- 1. the cast ----------------
struct TriRays {
    const float* origin; const float* dir; int stride, n;        // the generic form
    int pinhole, W, H, tiles_x, tiles_y;                          // the pinhole form: dir = (((float)x - cx) fxi, ((float)y - cy) fyi, 1)
    float fxi, fyi, cx, cy;
    int transform; float T[12];                                   // ray -> mesh, row-major 3 x 4, as TriQuery's
    double tmin, tmax;
    int gridded; float lo[3], hi[3]; int clo[3], chi[3];          // the gridded triangles' box and its cells
    double size;                                                  // max |box coordinate|
    float* t; int* tri; float* uv; unsigned char* front;
};
struct RayHit { double t, v, w; int tri; bool front; };
struct RayFrame { int kx, ky, kz; double ox, oy, oz, Sx, Sy, Sz; };   // o[kx], o[ky], o[kz]

__device__ __forceinline__ float ray_pick(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }
__device__ __forceinline__ int ray_picki(int x, int y, int z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

__device__ __forceinline__ void ray_test(const TriDev& m, unsigned t, const RayFrame& r, double tmin, double tmax, RayHit& best) {
    if ((int)t == best.tri) return;
    const float4 a = m.rec[(size_t)t * 3], b = m.rec[(size_t)t * 3 + 1], c = m.rec[(size_t)t * 3 + 2];
    const double az = (double)ray_pick(a.x, a.y, a.z, r.kz) - r.oz, bz = (double)ray_pick(b.x, b.y, b.z, r.kz) - r.oz, cz = (double)ray_pick(c.x, c.y, c.z, r.kz) - r.oz;
    const double Ax = ((double)ray_pick(a.x, a.y, a.z, r.kx) - r.ox) - r.Sx * az, Ay = ((double)ray_pick(a.x, a.y, a.z, r.ky) - r.oy) - r.Sy * az;
    const double Bx = ((double)ray_pick(b.x, b.y, b.z, r.kx) - r.ox) - r.Sx * bz, By = ((double)ray_pick(b.x, b.y, b.z, r.ky) - r.oy) - r.Sy * bz;
    const double Cx = ((double)ray_pick(c.x, c.y, c.z, r.kx) - r.ox) - r.Sx * cz, Cy = ((double)ray_pick(c.x, c.y, c.z, r.ky) - r.oy) - r.Sy * cz;
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return;
    const double det = (U + V) + W;
    if (det == 0.0) return;
    const double T = (U * (r.Sz * az) + V * (r.Sz * bz)) + W * (r.Sz * cz);
    const double tt = T / det;
    if (!(tt >= tmin && tt <= tmax)) return;
    if (best.tri < 0 || tt < best.t || (tt == best.t && (int)t < best.tri)) { best.t = tt; best.tri = (int)t; best.v = V / det; best.w = W / det; best.front = det > 0.0; }
}

// the minimum over (t, index) of the counting triangles for the ray (o, d) of the mesh's frame, finite and d != 0; best.tri = -1: none
__device__ __forceinline__ void ray_cast(const TriDev& m, const TriRays& a, float ox, float oy, float oz, float dx, float dy, float dz, RayHit& best) {
    RayFrame r;
    r.kz = 0;
    float big = fabsf(dx);
    if (fabsf(dy) > big) { r.kz = 1; big = fabsf(dy); }
    if (fabsf(dz) > big) r.kz = 2;
    r.kx = r.kz == 2 ? 0 : r.kz + 1; r.ky = r.kx == 2 ? 0 : r.kx + 1;
    const double dk = (double)ray_pick(dx, dy, dz, r.kz);
    if (dk < 0.0) { const int s = r.kx; r.kx = r.ky; r.ky = s; }
    r.Sx = (double)ray_pick(dx, dy, dz, r.kx) / dk; r.Sy = (double)ray_pick(dx, dy, dz, r.ky) / dk; r.Sz = 1.0 / dk;
    r.ox = (double)ray_pick(ox, oy, oz, r.kx); r.oy = (double)ray_pick(ox, oy, oz, r.ky); r.oz = (double)ray_pick(ox, oy, oz, r.kz);
    const double h = m.g.h, inv_h = m.g.inv_h;
    const double pad = h * kRayPadCell + (fmax(fabs(r.ox), fmax(fabs(r.oy), fabs(r.oz))) + a.size) * kRayPadSize;
    const double tm = 2.0 * pad * fabs(r.Sz);

    if (a.gridded) {
        const double lox = (double)ray_pick(a.lo[0], a.lo[1], a.lo[2], r.kx), hix = (double)ray_pick(a.hi[0], a.hi[1], a.hi[2], r.kx);
        const double loy = (double)ray_pick(a.lo[0], a.lo[1], a.lo[2], r.ky), hiy = (double)ray_pick(a.hi[0], a.hi[1], a.hi[2], r.ky);
        const int cxlo = ray_picki(a.clo[0], a.clo[1], a.clo[2], r.kx), cxhi = ray_picki(a.chi[0], a.chi[1], a.chi[2], r.kx);
        const int cylo = ray_picki(a.clo[0], a.clo[1], a.clo[2], r.ky), cyhi = ray_picki(a.chi[0], a.chi[1], a.chi[2], r.ky);
        const int czlo = ray_picki(a.clo[0], a.clo[1], a.clo[2], r.kz), czhi = ray_picki(a.chi[0], a.chi[1], a.chi[2], r.kz);
        // [z0, z1]: the box widened by one cell, [tmin, tmax], and the two minor slabs
        double z0 = (double)ray_pick(a.lo[0], a.lo[1], a.lo[2], r.kz) - h, z1 = (double)ray_pick(a.hi[0], a.hi[1], a.hi[2], r.kz) + h;
        const double za = r.oz + a.tmin * dk, zb = r.oz + a.tmax * dk;
        z0 = fmax(z0, fmin(za, zb) - pad); z1 = fmin(z1, fmax(za, zb) + pad);
        if (r.Sx != 0.0) {
            const double q0 = ((lox - h) - r.ox) / r.Sx, q1 = ((hix + h) - r.ox) / r.Sx;
            z0 = fmax(z0, r.oz + fmin(q0, q1)); z1 = fmin(z1, r.oz + fmax(q0, q1));
        } else if (r.ox < lox - h || r.ox > hix + h) z1 = -INFINITY;
        if (r.Sy != 0.0) {
            const double q0 = ((loy - h) - r.oy) / r.Sy, q1 = ((hiy + h) - r.oy) / r.Sy;
            z0 = fmax(z0, r.oz + fmin(q0, q1)); z1 = fmin(z1, r.oz + fmax(q0, q1));
        } else if (r.oy < loy - h || r.oy > hiy + h) z1 = -INFINITY;
        if (z0 <= z1) {
            const int Llo = (int)fmax(floor(z0 * inv_h), (double)czlo), Lhi = (int)fmin(floor(z1 * inv_h), (double)czhi);
            const bool fwd = dk > 0.0;
            for (int k = 0; k <= Lhi - Llo; ++k) {
                const int L = fwd ? Llo + k : Lhi - k;
                const double zlo = fmax((double)L * h - pad, z0), zhi = fmin((double)(L + 1) * h + pad, z1);
                if (((fwd ? zlo : zhi) - r.oz) * r.Sz - tm > best.t) break;
                const double xa = r.ox + r.Sx * (zlo - r.oz), xb = r.ox + r.Sx * (zhi - r.oz);
                const double ya = r.oy + r.Sy * (zlo - r.oz), yb = r.oy + r.Sy * (zhi - r.oz);
                const int x0 = (int)fmax(floor((fmin(xa, xb) - pad) * inv_h), (double)cxlo), x1 = (int)fmin(floor((fmax(xa, xb) + pad) * inv_h), (double)cxhi);
                const int y0 = (int)fmax(floor((fmin(ya, yb) - pad) * inv_h), (double)cylo), y1 = (int)fmin(floor((fmax(ya, yb) + pad) * inv_h), (double)cyhi);
                for (int cy = y0; cy <= y1; ++cy)
                    for (int cx = x0; cx <= x1; ++cx) {
                        const int gx = r.kx == 0 ? cx : (r.ky == 0 ? cy : L), gy = r.kx == 1 ? cx : (r.ky == 1 ? cy : L), gz = r.kx == 2 ? cx : (r.ky == 2 ? cy : L);
                        const unsigned bk = nn_hash(gx, gy, gz) & m.g.mask;
                        const unsigned e = m.g.start[bk + 1];
                        for (unsigned i = m.g.start[bk]; i < e; ++i) ray_test(m, m.items[i], r, a.tmin, a.tmax, best);
                    }
            }
        }
    }
    for (unsigned k = 0; k < m.n_wide; ++k) {
        const unsigned t = m.wide[k];
        const float4 A = m.rec[(size_t)t * 3], B = m.rec[(size_t)t * 3 + 1], C = m.rec[(size_t)t * 3 + 2];
        const float lz = ray_pick(fminf(A.x, fminf(B.x, C.x)), fminf(A.y, fminf(B.y, C.y)), fminf(A.z, fminf(B.z, C.z)), r.kz);
        const float hz = ray_pick(fmaxf(A.x, fmaxf(B.x, C.x)), fmaxf(A.y, fmaxf(B.y, C.y)), fmaxf(A.z, fmaxf(B.z, C.z)), r.kz);
        const double zlo = (double)lz - pad, zhi = (double)hz + pad;
        const double ta = (zlo - r.oz) * r.Sz, tb = (zhi - r.oz) * r.Sz;
        if (fmin(ta, tb) - tm > fmin(a.tmax, best.t) || fmax(ta, tb) + tm < a.tmin) continue;
        const double xa = r.ox + r.Sx * (zlo - r.oz), xb = r.ox + r.Sx * (zhi - r.oz);
        const double ya = r.oy + r.Sy * (zlo - r.oz), yb = r.oy + r.Sy * (zhi - r.oz);
        if (fmin(xa, xb) - pad > (double)ray_pick(fmaxf(A.x, fmaxf(B.x, C.x)), fmaxf(A.y, fmaxf(B.y, C.y)), fmaxf(A.z, fmaxf(B.z, C.z)), r.kx) ||
            fmax(xa, xb) + pad < (double)ray_pick(fminf(A.x, fminf(B.x, C.x)), fminf(A.y, fminf(B.y, C.y)), fminf(A.z, fminf(B.z, C.z)), r.kx) ||
            fmin(ya, yb) - pad > (double)ray_pick(fmaxf(A.x, fmaxf(B.x, C.x)), fmaxf(A.y, fmaxf(B.y, C.y)), fmaxf(A.z, fmaxf(B.z, C.z)), r.ky) ||
            fmax(ya, yb) + pad < (double)ray_pick(fminf(A.x, fminf(B.x, C.x)), fminf(A.y, fminf(B.y, C.y)), fminf(A.z, fminf(B.z, C.z)), r.ky))
            continue;
        ray_test(m, t, r, a.tmin, a.tmax, best);
    }
}

__global__ __launch_bounds__(kNnThreads) void k_tri_raycast(TriDev m, TriRays a) {
    const int lane = threadIdx.x & 63, waves = kNnThreads / 64;
    const int units = a.pinhole ? a.tiles_x * a.tiles_y : (a.n + 63) / 64;     // a wavefront's 64 rays: a tile, or 64 in a row
    for (int u = blockIdx.x * waves + (threadIdx.x >> 6); u < units; u += gridDim.x * waves) {
        int i;
        float ox = 0.f, oy = 0.f, oz = 0.f, dx, dy, dz;
        if (a.pinhole) {
            const int px = (u % a.tiles_x) * kRayTile + (lane & (kRayTile - 1)), py = (u / a.tiles_x) * kRayTile + lane / kRayTile;
            if (px >= a.W || py >= a.H) continue;
            i = py * a.W + px;
            dx = ((float)px - a.cx) * a.fxi; dy = ((float)py - a.cy) * a.fyi; dz = 1.f;    // k_vmap_nmap's vertex of depth 1
        } else {
            i = u * 64 + lane;
            if (i >= a.n) continue;
            const float* po = a.origin + (size_t)i * a.stride; const float* pd = a.dir + (size_t)i * a.stride;
            ox = po[0]; oy = po[1]; oz = po[2]; dx = pd[0]; dy = pd[1]; dz = pd[2];
        }
        if (a.transform) {   // mf_cloud_nn_dev's transform, bit for bit; the direction by the linear part alone
            const float tx = a.T[0] * ox + a.T[1] * oy + a.T[2] * oz + a.T[3];
            const float ty = a.T[4] * ox + a.T[5] * oy + a.T[6] * oz + a.T[7];
            const float tz = a.T[8] * ox + a.T[9] * oy + a.T[10] * oz + a.T[11];
            const float ex = a.T[0] * dx + a.T[1] * dy + a.T[2] * dz;
            const float ey = a.T[4] * dx + a.T[5] * dy + a.T[6] * dz;
            const float ez = a.T[8] * dx + a.T[9] * dy + a.T[10] * dz;
            ox = tx; oy = ty; oz = tz; dx = ex; dy = ey; dz = ez;
        }
        RayHit best;
        best.t = INFINITY; best.v = best.w = 0.0; best.tri = -1; best.front = false;
        if (nn_finite(ox, oy, oz) && nn_finite(dx, dy, dz) && !(dx == 0.f && dy == 0.f && dz == 0.f) && m.nt > 0) ray_cast(m, a, ox, oy, oz, dx, dy, dz, best);
        const bool hit = best.tri >= 0;
        a.t[i] = hit ? (float)best.t : (a.pinhole ? 0.f : INFINITY);
        a.tri[i] = best.tri;
        if (a.uv) { a.uv[(size_t)i * 2] = hit ? (float)best.v : NAN; a.uv[(size_t)i * 2 + 1] = hit ? (float)best.w : NAN; }
        if (a.front) a.front[i] = hit && best.front ? 1 : 0;
    }
}

// the checks the two calls share, and the launch
static int ray_launch(const mf_trimesh* h, TriRays& a, const float* T16, float tmin, float tmax, int64_t rays, void* stream) {
    if (!std::isfinite(tmin)) return tri_fail("tmin must be finite", MF_EINVAL);
    if (std::isnan(tmax) || tmax < tmin) return tri_fail("tmax must be >= tmin (it may be +inf)", MF_EINVAL);
    if (T16)
        for (int k = 0; k < 16; ++k)
            if (!std::isfinite(T16[k])) return tri_fail("transform is not finite", MF_EINVAL);
    TriDev m = h->m;
    a.gridded = h->gridded ? 1 : 0;
    a.size = 0.0;
    for (int k = 0; k < 3 && h->gridded; ++k) {
        a.lo[k] = h->lo[k]; a.hi[k] = h->hi[k];
        a.clo[k] = (int)floor((double)h->lo[k] * m.g.inv_h); a.chi[k] = (int)floor((double)h->hi[k] * m.g.inv_h);   // nn_cell
        if ((long long)a.chi[k] - (long long)a.clo[k] + 1 > kRayMaxLayerCells)
            return tri_fail("the mesh spans more than 2^15 cells on an axis: build it with a larger cell", MF_EINVAL);
        a.size = std::max(a.size, std::max(std::fabs((double)h->lo[k]), std::fabs((double)h->hi[k])));
    }
    if (rays == 0) return MF_OK;
    a.tmin = (double)tmin; a.tmax = (double)tmax;
    if (T16) {
        a.transform = 1;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) a.T[r * 4 + c] = T16[c * 4 + r];
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t units = a.pinhole ? (int64_t)a.tiles_x * a.tiles_y : (rays + 63) / 64;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((units + kNnThreads / 64 - 1) / (kNnThreads / 64), kNnMaxGrid));
    hipLaunchKernelGGL(k_tri_raycast, dim3(blocks), dim3(kNnThreads), 0, s, m, a);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return tri_fail("HIP error during the ray kernel", MF_EHIP);
    return MF_OK;
}

}  // namespace mf

using namespace mf;

extern "C" int mf_trimesh_raycast_dev(const mf_trimesh* h, const float* d_origin, const float* d_dir, int32_t ray_stride, int64_t n_rays,
                                      const float* ray_to_mesh16, float tmin, float tmax, float* d_t, int32_t* d_tri, float* d_uv, uint8_t* d_front,
                                      void* stream) {
    if (!h) return tri_fail("null handle", MF_EINVAL);
    if (n_rays < 0 || n_rays > (int64_t)1 << 30) return tri_fail("ray count out of range (0 .. 2^30)", MF_EINVAL);
    if (n_rays > 0 && (!d_origin || !d_dir || !d_t || !d_tri)) return tri_fail("null rays or outputs", MF_EINVAL);
    if (ray_stride < 3) return tri_fail("ray_stride must be >= 3 floats", MF_EINVAL);
    TriRays a;
    memset(&a, 0, sizeof(a));
    a.origin = d_origin; a.dir = d_dir; a.stride = ray_stride; a.n = (int)n_rays;
    a.t = d_t; a.tri = d_tri; a.uv = d_uv; a.front = d_front;
    return ray_launch(h, a, ray_to_mesh16, tmin, tmax, n_rays, stream);
}

extern "C" int mf_trimesh_render_dev(const mf_trimesh* h, int32_t width, int32_t height, float fx, float fy, float cx, float cy,
                                     const float* mesh_from_cam16, float tmin, float tmax, float* d_depth, int32_t* d_tri, float* d_uv,
                                     uint8_t* d_front, void* stream) {
    if (!h) return tri_fail("null handle", MF_EINVAL);
    if (width < 1 || width > 16384 || height < 1 || height > 16384) return tri_fail("width and height must be 1 .. 16384", MF_EINVAL);
    if (!d_depth || !d_tri || !mesh_from_cam16) return tri_fail("null outputs or transform", MF_EINVAL);
    if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.f || fy == 0.f || !std::isfinite(cx) || !std::isfinite(cy))
        return tri_fail("fx, fy must be finite and not 0, cx, cy finite", MF_EINVAL);
    TriRays a;
    memset(&a, 0, sizeof(a));
    a.pinhole = 1; a.W = width; a.H = height; a.tiles_x = (width + kRayTile - 1) / kRayTile; a.tiles_y = (height + kRayTile - 1) / kRayTile;
    a.fxi = 1.f / fx; a.fyi = 1.f / fy; a.cx = cx; a.cy = cy;
    a.t = d_depth; a.tri = d_tri; a.uv = d_uv; a.front = d_front;
    return ray_launch(h, a, mesh_from_cam16, tmin, tmax, (int64_t)width * height, stream);
}
