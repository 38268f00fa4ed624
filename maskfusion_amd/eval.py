"""Run evaluation: trajectories (TUM-style ATE / RPE) and maps (accuracy / completeness / F-score by GPU nearest-surfel distances).

Reads what a run writes -- poses-<id>.txt (mf_export_poses; TUM `ts tx ty tz qx qy qz qw`, also a TUM groundtruth.txt) and cloud-<id>.ply
(mf_save_ply; binary little endian, or ASCII PLY with x / y / z) -- from this library or from the reference.  The cloud distances run on the
GPU through mf_cloud_nn_dev (kernels: csrc/mf_eval.hip); everything else is numpy.  register() refines the rigid alignment of two clouds
before they are scored: point-to-plane (or point-to-point) Gauss-Newton steps on the GPU (mf_cloud_icp_build_dev / mf_cloud_icp_step_dev), the
6 x 6 solve and the pose update in fp64 here.  estimate_normals() gives a cloud that has no normals the ones point-to-plane needs, from its
own radius neighbourhoods on the GPU (mf_cloud_normals_dev); normal_consistency() scores the normals of two clouds against each other.
register_global() needs no start: FPFH descriptors of voxel key points (mf_cloud_fpfh_dev) matched on the GPU (mf_feature_match_dev), a
seeded RANSAC over the matches in numpy, then register().

    python -m maskfusion_amd.eval --est DIR [--ref DIR] [--gt FILE] [--radius R] [--tau a,b,c] [--pair est_id:ref_id ...]
                                  [--register [--register-radius R0,R1,...] [--register-iterations N] [--point-to-point]]
                                  [--register-global[=VOXEL]] [--ref-cloud FILE [--init FILE]] [--estimate-normals[=R]] [--normals]
                                  [--ref-mesh FILE [--mesh-density D] [--mesh-cell C]]
                                  [--seg-gt DIR [--seg-gt-prefix Mask] [--seg-index-width 4] [--seg-radius R] [--seg-void V]]
                                  [--observed-from SEQ [--observed-poses FILE] [--observed-cal FILE] [--observed-tol A[,R]]
                                   [--observed-rule seen|surface] [--observed-min-frames K] [--observed-stride S] [--observed-max-depth D]
                                   [--observed-time-scale S]]

prints one JSON object per model on stdout (INTEGRATION.md "Evaluating a run"); with --seg-gt, one per ground-truth object of the
segmentation and a summary (region similarity J and boundary accuracy F of the -es label images, counted on the GPU:
mf_label_confusion_dev / mf_label_boundary_dev).  ViewScorer scores what needs nothing from outside the run: the map's render from the
sensor's own view against the frame it just saw (mf_view_score_dev; the driver's -evalviews flag writes its result as views.json).
With --observed-from, completeness and F-score are also reported over the part of the reference the sequence observed: every reference point
is classified against every depth frame on the GPU (mf_cloud_visibility_dev; Visibility, observed, observe_sequence).
With --ref-mesh the reference is a triangle mesh (.ply or .obj): accuracy is the exact distance to its triangles and its area-uniform samples
stand in for the reference cloud everywhere else (TriMesh, compare_cloud_mesh; mf_trimesh_*, kernels: csrc/mf_eval_trimesh.hip).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import re
import sys

import numpy as np

# ------------------------------------------------------------------------------------------------------------------------------------
# trajectories
# ------------------------------------------------------------------------------------------------------------------------------------


def quat_to_rot(q) -> np.ndarray:
    """(qx, qy, qz, qw) -> 3 x 3 (normalised first)"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def read_tum(path: str):
    """poses-<id>.txt or a TUM groundtruth.txt: `ts tx ty tz qx qy qz qw` per line, `#` comments, blank lines ignored (commas count as
    blanks).  Returns (timestamps float64 [n], poses float64 [n, 4, 4]) in file order."""
    ts, T = [], []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].replace(",", " ").strip()
            if not line:
                continue
            v = [float(x) for x in line.split()]
            if len(v) < 8:
                raise ValueError(f"{path}: expected 8 numbers per line, got {len(v)}: {line!r}")
            M = np.eye(4)
            M[:3, :3] = quat_to_rot(v[4:8])
            M[:3, 3] = v[1:4]
            ts.append(v[0])
            T.append(M)
    return np.array(ts, np.float64), np.array(T, np.float64).reshape(-1, 4, 4)


def associate(a, b, max_dt: float = 0.02):
    """TUM associate.py: the candidate pairs (i, j) with |a[i] - b[j]| < max_dt, taken greedily by the smallest |dt| with every stamp used at
    most once.  Returns the pairs as an int array [m, 2], sorted by i."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    order = np.argsort(b, kind="stable")
    bs = b[order]
    cand = []
    for i, t in enumerate(a):
        lo, hi = np.searchsorted(bs, t - max_dt, "left"), np.searchsorted(bs, t + max_dt, "right")
        for k in range(lo, hi):
            d = abs(t - bs[k])
            if d < max_dt:
                cand.append((d, i, int(order[k])))
    cand.sort()
    used_a, used_b, out = set(), set(), []
    for _, i, j in cand:
        if i in used_a or j in used_b:
            continue
        used_a.add(i)
        used_b.add(j)
        out.append((i, j))
    out.sort()
    return np.array(out, np.int64).reshape(-1, 2)


def align_horn(est, gt) -> np.ndarray:
    """Rigid alignment without scale (Horn / Umeyama, s = 1): the 4 x 4 T minimising sum |T est_k - gt_k|^2 over (n, 3) point lists."""
    est = np.asarray(est, np.float64)
    gt = np.asarray(gt, np.float64)
    me, mg = est.mean(0), gt.mean(0)
    H = (est - me).T @ (gt - mg)
    U, _, Vt = np.linalg.svd(H)
    D = np.eye(3)
    if np.linalg.det(Vt.T @ U.T) < 0:
        D[2, 2] = -1.0
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mg - R @ me
    return T


def _stats(e):
    e = np.asarray(e, np.float64)
    if e.size == 0:
        return {"rmse": None, "mean": None, "median": None, "std": None, "min": None, "max": None}
    return {"rmse": float(np.sqrt((e * e).mean())), "mean": float(e.mean()), "median": float(np.median(e)), "std": float(e.std()),
            "min": float(e.min()), "max": float(e.max())}


def ate(est, gt, max_dt: float = 0.02) -> dict:
    """Absolute trajectory error (TUM evaluate_ate.py): est and gt are read_tum() results; the associated positions are aligned rigidly
    (align_horn, est -> gt) and the statistics are those of the translational residuals (m)."""
    pairs = associate(est[0], gt[0], max_dt)
    out = {"pairs": int(len(pairs))}
    if len(pairs) == 0:
        out.update(_stats([]))
        return out
    pe = est[1][pairs[:, 0], :3, 3]
    pg = gt[1][pairs[:, 1], :3, 3]
    T = align_horn(pe, pg) if len(pairs) >= 3 else np.eye(4)
    r = np.linalg.norm(pe @ T[:3, :3].T + T[:3, 3] - pg, axis=1)
    out.update(_stats(r))
    out["alignment"] = T.tolist()
    return out


def _closest(xs, x) -> int:
    """TUM's find_closest_index: binary search over sorted xs, the first strictly closer element found wins (an exact hit at once)"""
    lo, hi, best, diff = 0, len(xs), 0, abs(xs[0] - x)
    while lo < hi:
        mid = (lo + hi) // 2
        if abs(xs[mid] - x) < diff:
            diff, best = abs(xs[mid] - x), mid
        if xs[mid] == x:
            return mid
        if xs[mid] > x:
            hi = mid
        else:
            lo = mid + 1
    return best


def rpe(est, gt, delta: float = 1.0, unit: str = "s") -> dict:
    """Relative pose error as TUM evaluate_rpe.py --fixed_delta computes it (every pair, no sampling): over est's poses in stamp order,
    pose i's partner j is the pose whose stamp (unit "s") or position (unit "f") is closest to its own + delta, skipped when j is the last
    pose; each of the two takes the gt pose with the closest stamp, and the pair is skipped when either lies more than twice the median gt
    interval away.  Error = ominus(ominus(est_j, est_i), ominus(gt_j, gt_i)) = (est_i^-1 est_j) (gt_i^-1 gt_j)^-1 with ominus(a, b) = a^-1 b.
    Returns the translational RMSE and mean (m) and the mean rotation angle (deg)."""
    if unit not in ("s", "f"):
        raise ValueError("unit must be 's' or 'f'")
    oe, og = np.argsort(est[0], kind="stable"), np.argsort(gt[0], kind="stable")
    se, E = est[0][oe], est[1][oe]
    sg, G = gt[0][og], gt[1][og]
    te, re_ = [], []
    if len(se) >= 2 and len(sg) >= 2:
        index = se if unit == "s" else np.arange(len(se), dtype=np.float64)
        max_gt_dt = 2.0 * float(np.median(np.diff(sg)))
        for i in range(len(se)):
            j = _closest(index, index[i] + delta)
            if j == len(se) - 1:
                continue
            gi, gj = _closest(sg, se[i]), _closest(sg, se[j])
            if abs(sg[gi] - se[i]) > max_gt_dt or abs(sg[gj] - se[j]) > max_gt_dt:
                continue
            err = (np.linalg.inv(E[i]) @ E[j]) @ np.linalg.inv(np.linalg.inv(G[gi]) @ G[gj])
            te.append(np.linalg.norm(err[:3, 3]))
            re_.append(math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(err[:3, :3]) - 1.0) / 2.0)))))
    te = np.array(te)
    return {"pairs": int(len(te)), "delta": delta, "unit": unit,
            "trans_rmse": float(np.sqrt((te * te).mean())) if len(te) else None,
            "trans_mean": float(te.mean()) if len(te) else None,
            "rot_mean_deg": float(np.mean(re_)) if len(te) else None}


# ------------------------------------------------------------------------------------------------------------------------------------
# clouds
# ------------------------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path: str, normals: bool = False):
    """The vertex positions of a PLY file, (n, 3) float32: binary little endian (mf_save_ply's and the reference's layout) or ASCII.
    The vertex element must come first; other elements after it are ignored.  normals=True: (positions, normals) with the file's
    nx / ny / nz as (n, 3) float32 (mf_save_ply writes them), or None in their place when the file has none."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body_at = raw.index(b"\n", end) + 1
    fmt, elems = None, []
    for line in raw[:end].decode("ascii", "replace").splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elems.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elems:
            if w[1] == "list":
                elems[-1][2].append((w[-1], None))
            else:
                elems[-1][2].append((w[2], _PLY_TYPES[w[1]]))
    if not elems or elems[0][0] != "vertex":
        raise ValueError(f"{path}: the first element is not 'vertex'")
    _, n, props = elems[0]
    names = [p[0] for p in props]
    if not all(k in names for k in ("x", "y", "z")) or any(t is None for _, t in props):
        raise ValueError(f"{path}: vertices need x, y, z and no list properties")
    has_n = all(k in names for k in ("nx", "ny", "nz"))
    if fmt == "binary_little_endian":
        dt = np.dtype([(nm, "<" + t) for nm, t in props])
        v = np.frombuffer(raw, dt, count=n, offset=body_at)
        xyz = np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)
        if not normals:
            return xyz
        return xyz, (np.stack([v["nx"], v["ny"], v["nz"]], 1).astype(np.float32) if has_n else None)
    if fmt == "ascii":
        lines = raw[body_at:].decode("ascii").split("\n")
        rows = [l.split() for l in lines if l.strip()][:n]
        a = np.array(rows, np.float64).reshape(n, len(props))
        xyz = a[:, [names.index("x"), names.index("y"), names.index("z")]].astype(np.float32)
        if not normals:
            return xyz
        return xyz, (a[:, [names.index("nx"), names.index("ny"), names.index("nz")]].astype(np.float32) if has_n else None)
    raise ValueError(f"{path}: format {fmt} is not supported")


def _device_points(a, min_cols: int = 3, what: str = "points must be (n, >= 3) float32"):
    """(n, >= min_cols) float32 as a contiguous tensor on the library's device"""
    import torch
    from .lib import torch_device
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32)))
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < min_cols:
        raise ValueError(what)
    return t.to(torch_device()).contiguous()


def _stream_of(device):
    """the handle of torch's current stream on `device` as the library takes it: None off the GPU"""
    import torch
    return torch.cuda.current_stream().cuda_stream if device.type == "cuda" else None


def _pack_T(T):
    """a 4 x 4 transform as the 16 column-major floats the library takes, or None"""
    return None if T is None else np.ascontiguousarray(np.asarray(T, np.float32).T.reshape(16))


def _workspace(L, name: str, device, *counts):
    """(uint8 tensor on `device`, its size in bytes): what the library's function `name` asks for `counts` points"""
    import torch
    from .lib import MFError
    need = C.c_uint64(0)
    if getattr(L, name)(*counts, C.byref(need)) != 0:
        raise MFError(f"{name} failed")
    return torch.empty(int(need.value), dtype=torch.uint8, device=device), int(need.value)


def _check(rc: int, name: str, hint: str):
    from .lib import MFError
    if rc != 0:
        raise MFError(f"{name} failed with code {rc} ({hint})")


def nearest(target, query, radius: float, T=None):
    """For every query point the nearest target point within `radius` (mf_cloud_nn_dev on device buffers).  target, query: (n, >= 3)
    float32 numpy arrays or device tensors (x, y, z first); T: 4 x 4 applied to the queries first.  Returns numpy (dist float32, +inf: none
    in range; idx int32, -1: none)."""
    import torch
    from .lib import load
    L = load()
    t, q = _device_points(target), _device_points(query)
    nt, nq = int(t.shape[0]), int(q.shape[0])
    ws, need = _workspace(L, "mf_cloud_nn_workspace", q.device, nt)
    dist = torch.empty(max(nq, 1), dtype=torch.float32, device=q.device)
    idx = torch.empty(max(nq, 1), dtype=torch.int32, device=q.device)
    T16 = _pack_T(T)
    rc = L.mf_cloud_nn_dev(t.data_ptr() if nt else None, int(t.shape[1]), nt, q.data_ptr() if nq else None, int(q.shape[1]), nq,
                           T16.ctypes.data if T16 is not None else None, float(radius), dist.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                           need, _stream_of(q.device))
    _check(rc, "mf_cloud_nn_dev", "radius must be finite and > 0, coordinates |x / radius| < 2^30")
    return dist[:nq].cpu().numpy(), idx[:nq].cpu().numpy()


def cloud_stats(dist, radius: float, taus) -> dict:
    """count, misses (nothing within radius), mean / RMSE / median of min(d, radius), and the fraction <= tau for every tau"""
    d = np.asarray(dist, np.float64)
    c = np.minimum(d, radius)
    out = {"count": int(d.size), "misses": int(np.count_nonzero(~np.isfinite(d)))}
    if d.size:
        out.update({"mean": float(c.mean()), "rmse": float(np.sqrt((c * c).mean())), "median": float(np.median(c))})
    else:
        out.update({"mean": None, "rmse": None, "median": None})
    out["fraction"] = {f"{t:g}": (float(np.count_nonzero(d <= t)) / d.size if d.size else 0.0) for t in taus}
    return out


def transform_f32(T, pts) -> np.ndarray:
    """mf_cloud_nn_dev's query transform, on the host and with the same bits: x' = ((T00 x + T01 y) + T02 z) + T03 in fp32"""
    T = np.asarray(T, np.float32)
    p = np.asarray(pts, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([T[r, 0] * x + T[r, 1] * y + T[r, 2] * z + T[r, 3] for r in range(3)], 1)


def compare_clouds(est, ref, radius: float = 0.05, taus=(0.01, 0.02, 0.05), T=None, ref_keep=None) -> dict:
    """accuracy = est -> ref distances, completeness = ref -> est, and F-score(tau) = 2 P R / (P + R) with P, R their fractions <= tau.
    T (4 x 4, est -> ref; e.g. register()'s): est is moved by it first (transform_f32), for both directions.
    ref_keep (bool per reference point, e.g. observed()'s; None: all): completeness is taken over ref[ref_keep] only -- the part of the
    reference the sensor observed.  Accuracy is still measured against the whole reference: an estimate point that lies on reference surface
    the mask leaves out is not an error."""
    if T is not None:
        est = transform_f32(T, est.cpu().numpy() if hasattr(est, "cpu") else est)
    acc = cloud_stats(nearest(ref, est, radius)[0], radius, taus)
    if ref_keep is not None:
        keep = np.asarray(ref_keep)
        if keep.dtype != np.bool_ or keep.shape != (len(ref),):
            raise ValueError("ref_keep must be one bool per reference point")
        if hasattr(ref, "cpu"):
            import torch
            ref = ref[torch.as_tensor(keep).to(ref.device)]
        else:
            ref = np.asarray(ref)[keep]
    comp = cloud_stats(nearest(est, ref, radius)[0], radius, taus)
    f = {}
    for t in taus:
        k = f"{t:g}"
        p, r = acc["fraction"][k], comp["fraction"][k]
        f[k] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return {"radius": radius, "accuracy": acc, "completeness": comp, "fscore": f}


class TriMesh:
    """The library's handle of a triangle mesh to score against (mf_trimesh; include/maskfusion_amd.h has the definitions): distance() is the
    exact distance to the nearest triangle, sample() the deterministic area-uniform sampler.  vertices (n, >= 3) float32, triangles (m, 3)
    int32 -- numpy arrays or device tensors; cell: the edge of the search structure's cells (speed only; radius <= 16 cell).  A context
    manager, like mesh.Mesh."""

    def __init__(self, vertices, triangles, cell: float):
        import torch
        from .lib import MFError, load
        self._L = load()
        self._h = C.c_void_p()
        v = _device_points(vertices, 3, "vertices must be (n, >= 3) float32")
        t = triangles if isinstance(triangles, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(triangles, np.int32)).reshape(-1, 3))
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("triangles must be (m, 3) int32")
        t = t.to(v.device).contiguous()
        self.device = v.device
        self._stream = _stream_of(v.device)
        nv, nt = int(v.shape[0]), int(t.shape[0])
        ne = C.c_uint32(0)
        rc = self._L.mf_trimesh_build_dev(v.data_ptr() if nv else None, int(v.shape[1]), nv, t.data_ptr() if nt else None, nt, float(cell),
                                          C.byref(self._h), C.byref(ne), self._stream)
        if rc != 0:
            raise MFError(f"mf_trimesh_build_dev failed with code {rc}: {self._L.mf_last_error(None).decode()}")
        self.n_triangles, self.n_eligible, self.cell, self.density = nt, int(ne.value), float(cell), None

    def _fail(self, name, rc):
        from .lib import MFError
        raise MFError(f"{name} failed with code {rc}: {self._L.mf_last_error(None).decode()}")

    def distance(self, query, radius: float, T=None, closest: bool = False):
        """numpy (dist float32, +inf: no triangle within radius; tri int32, -1: none[; closest (n, 3) float32, NaN: none]) for every query
        point; T: 4 x 4 applied to the queries first, as nearest()'s"""
        import torch
        q = _device_points(query)
        nq = int(q.shape[0])
        dist = torch.empty(max(nq, 1), dtype=torch.float32, device=q.device)
        tri = torch.empty(max(nq, 1), dtype=torch.int32, device=q.device)
        cl = torch.empty((max(nq, 1), 3), dtype=torch.float32, device=q.device) if closest else None
        T16 = _pack_T(T)
        rc = self._L.mf_trimesh_distance_dev(self._h, q.data_ptr() if nq else None, int(q.shape[1]), nq, T16.ctypes.data if T16 is not None else None,
                                             float(radius), dist.data_ptr(), tri.data_ptr(), cl.data_ptr() if closest else None, self._stream)
        if rc != 0:
            self._fail("mf_trimesh_distance_dev", rc)
        out = (dist[:nq].cpu().numpy(), tri[:nq].cpu().numpy())
        return out + (cl[:nq].cpu().numpy(),) if closest else out

    def sample(self, density: float):
        """numpy (points (n, 3) float32, unit face normals (n, 3) float32, triangle index int32 (n,)) of the sampler at `density` samples
        per unit area"""
        import torch
        n = C.c_uint64(0)
        rc = self._L.mf_trimesh_sample_plan_dev(self._h, float(density), C.byref(n), self._stream)
        if rc != 0:
            self._fail("mf_trimesh_sample_plan_dev", rc)
        n = int(n.value)
        p = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
        nr = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
        tri = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        rc = self._L.mf_trimesh_sample_emit_dev(self._h, p.data_ptr(), nr.data_ptr(), tri.data_ptr(), self._stream)
        if rc != 0:
            self._fail("mf_trimesh_sample_emit_dev", rc)
        self.density = float(density)
        return p[:n].cpu().numpy(), nr[:n].cpu().numpy(), tri[:n].cpu().numpy()

    def raycast(self, origins, dirs, T=None, tmin: float = 0.0, tmax: float = float("inf")):
        """numpy (t float32, +inf: no hit; tri int32, -1: none; uv (n, 2) float32, the weights of the triangle's b and c, NaN: none; front
        bool: the ray met the counter-clockwise side) of the first triangle each ray origins[i] + t dirs[i] hits with tmin <= t <= tmax
        (mf_trimesh_raycast_dev); T: 4 x 4 applied to the rays first, the directions by its linear part"""
        import torch
        o, d = _device_points(origins), _device_points(dirs)
        if o.shape != d.shape:
            raise ValueError("origins and dirs must have one shape")
        n = int(o.shape[0])
        t = torch.empty(max(n, 1), dtype=torch.float32, device=o.device)
        tri = torch.empty(max(n, 1), dtype=torch.int32, device=o.device)
        uv = torch.empty((max(n, 1), 2), dtype=torch.float32, device=o.device)
        front = torch.empty(max(n, 1), dtype=torch.uint8, device=o.device)
        T16 = _pack_T(T)
        rc = self._L.mf_trimesh_raycast_dev(self._h, o.data_ptr() if n else None, d.data_ptr() if n else None, int(o.shape[1]), n,
                                            T16.ctypes.data if T16 is not None else None, float(tmin), float(tmax), t.data_ptr(), tri.data_ptr(),
                                            uv.data_ptr(), front.data_ptr(), self._stream)
        if rc != 0:
            self._fail("mf_trimesh_raycast_dev", rc)
        return t[:n].cpu().numpy(), tri[:n].cpu().numpy(), uv[:n].cpu().numpy(), front[:n].cpu().numpy().astype(bool)

    def render(self, W: int, H: int, fx: float, fy: float, cx: float, cy: float, mesh_from_cam, tmin: float = 0.0, tmax: float = float("inf")):
        """numpy (depth (H, W) float32, 0: nothing hit; tri (H, W) int32; uv (H, W, 2) float32; front (H, W) bool) of the mesh seen by the
        pinhole camera whose pose in the mesh's frame is mesh_from_cam (4 x 4): mf_trimesh_render_dev"""
        import torch
        W, H = int(W), int(H)
        n = max(W, 1) * max(H, 1)
        depth = torch.empty(n, dtype=torch.float32, device=self.device)
        tri = torch.empty(n, dtype=torch.int32, device=self.device)
        uv = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        front = torch.empty(n, dtype=torch.uint8, device=self.device)
        T16 = _pack_T(mesh_from_cam)
        rc = self._L.mf_trimesh_render_dev(self._h, W, H, float(fx), float(fy), float(cx), float(cy), T16.ctypes.data if T16 is not None else None,
                                           float(tmin), float(tmax), depth.data_ptr(), tri.data_ptr(), uv.data_ptr(), front.data_ptr(), self._stream)
        if rc != 0:
            self._fail("mf_trimesh_render_dev", rc)
        return (depth.cpu().numpy().reshape(H, W), tri.cpu().numpy().reshape(H, W), uv.cpu().numpy().reshape(H, W, 2),
                front.cpu().numpy().reshape(H, W).astype(bool))

    def close(self):
        if self._h:
            self._L.mf_trimesh_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def compare_cloud_mesh(est, trimesh, samples, radius: float = 0.05, taus=(0.01, 0.02, 0.05), T=None, ref_keep=None) -> dict:
    """compare_clouds against a triangle mesh: accuracy = est -> triangles (TriMesh.distance: exact, free of the sampling's bias),
    completeness = samples -> est (nearest; samples: TriMesh.sample()'s points), the same F-score, plus "reference".  T and ref_keep (one
    bool per sample) as in compare_clouds."""
    if T is not None:
        est = transform_f32(T, est.cpu().numpy() if hasattr(est, "cpu") else est)
    acc = cloud_stats(trimesh.distance(est, radius)[0], radius, taus)
    ref = samples.cpu().numpy() if hasattr(samples, "cpu") else np.asarray(samples, np.float32)
    n_samples = len(ref)
    if ref_keep is not None:
        keep = np.asarray(ref_keep)
        if keep.dtype != np.bool_ or keep.shape != (len(ref),):
            raise ValueError("ref_keep must be one bool per sample")
        ref = ref[keep]
    comp = cloud_stats(nearest(est, ref, radius)[0], radius, taus)
    f = {}
    for t in taus:
        k = f"{t:g}"
        p, r = acc["fraction"][k], comp["fraction"][k]
        f[k] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return {"radius": radius, "accuracy": acc, "completeness": comp, "fscore": f,
            "reference": {"triangles": trimesh.n_triangles, "eligible": trimesh.n_eligible, "samples": n_samples, "density": trimesh.density}}


# ------------------------------------------------------------------------------------------------------------------------------------
# registration
# ------------------------------------------------------------------------------------------------------------------------------------
class Registration:
    """The device side of register(): the reference cloud's grid for one radius (mf_cloud_icp_build_dev) and the Gauss-Newton system of a
    query cloud under a transform (mf_cloud_icp_step_dev).  ref: (n, >= 3) float32 array or device tensor, x, y, z first; normals: None
    (point-to-point), an (n, 3) array, or the column of ref where nx, ny, nz start (8 for mf_download_map's records)."""

    def __init__(self, ref, radius: float, normals=None, n_query: int = 0):
        import torch
        from .lib import load
        self._L = load()
        t = _device_points(ref)
        if normals is None:
            off = -1
        elif isinstance(normals, (int, np.integer)):
            off = int(normals)
        else:
            nr = _device_points(normals)
            if nr.shape[0] != t.shape[0]:
                raise ValueError("normals must have one row per reference point")
            t, off = torch.cat([t[:, :3], nr[:, :3]], 1).contiguous(), 3
        self.target, self.plane, self.radius = t, off >= 0, float(radius)
        self.n_query = int(n_query)
        nt = int(t.shape[0])
        self._ws, self._need = _workspace(self._L, "mf_cloud_icp_workspace", t.device, nt, self.n_query)
        self._out = torch.zeros(29, dtype=torch.float64, device=t.device)
        self._stream = lambda: _stream_of(t.device)
        rc = self._L.mf_cloud_icp_build_dev(t.data_ptr() if nt else None, int(t.shape[1]), off, nt, self.radius, self._ws.data_ptr(), self._need,
                                            self._stream())
        _check(rc, "mf_cloud_icp_build_dev", "radius must be finite and > 0, coordinates |x / radius| < 2^30, normals inside the record")

    def step(self, query, T=None) -> np.ndarray:
        """sys29 (float64 [29], see unpack_sys29) of `query` (device tensor or array, at most n_query points) mapped by T (4 x 4 or None)"""
        from .lib import MFError
        q = _device_points(query)
        nq = int(q.shape[0])
        if nq > self.n_query:
            raise MFError(f"{nq} queries, but the workspace was sized for {self.n_query}")
        T16 = _pack_T(T)
        rc = self._L.mf_cloud_icp_step_dev(self._ws.data_ptr(), self._need, q.data_ptr() if nq else None, int(q.shape[1]), nq,
                                           T16.ctypes.data if T16 is not None else None, self._out.data_ptr(), self._stream())
        _check(rc, "mf_cloud_icp_step_dev", f"finite transform, at most {self.n_query} queries, coordinates |x / radius| < 2^30")
        return self._out.cpu().numpy().copy()


def unpack_sys29(sys29):
    """(A = J^T J 6 x 6, b = J^T r, sum r^2, correspondences) from the packed upper triangle (mf_k_gn_solve's layout)"""
    s = np.asarray(sys29, np.float64)
    A, b, k = np.zeros((6, 6)), np.zeros(6), 0
    for i in range(6):
        for j in range(i, 7):
            if j == 6:
                b[i] = s[k]
            else:
                A[i, j] = A[j, i] = s[k]
            k += 1
    return A, b, float(s[27]), int(s[28])


def solve_step(sys29):
    """The Gauss-Newton step x = (t, w) with J^T J x = -J^T r by an unpivoted LDL^T in fp64, or (None, reason) outside the solver's stated
    domain (DESIGN.md finding F4): fewer than 6 correspondences, or a smallest pivot below 1e-8 of the largest diagonal entry."""
    A, b, _, n = unpack_sys29(sys29)
    if n < 6:
        return None, f"fewer than 6 correspondences ({n})"
    maxdiag = float(np.abs(np.diag(A)).max())
    Lm, D = np.eye(6), np.zeros(6)
    for j in range(6):
        D[j] = A[j, j] - float((Lm[j, :j] ** 2) @ D[:j])
        if not (D[j] >= 1e-8 * maxdiag and D[j] > 0.0):
            return None, (f"the system is rank deficient: pivot {j} is {D[j]:.3g}, below 1e-8 of the largest diagonal entry {maxdiag:.3g} "
                          "(the surface does not constrain all six degrees of freedom)")
        for i in range(j + 1, 6):
            Lm[i, j] = (A[i, j] - float((Lm[i, :j] * Lm[j, :j]) @ D[:j])) / D[j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = -b[i] - float(Lm[i, :i] @ y[:i])
    y /= D
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = y[i] - float(Lm[i + 1:, i] @ x[i + 1:])
    return x, None


def rodrigues(w) -> np.ndarray:
    """exp of the rotation vector w, 3 x 3"""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)


def update_se3(T, x) -> np.ndarray:
    """T <- [exp(w) | t] T with x = (t, w): the tracker's twist convention (computeUpdateSE3)"""
    U = np.eye(4)
    U[:3, :3] = rodrigues(x[3:])
    U[:3, 3] = x[:3]
    return U @ np.asarray(T, np.float64)


def rotation_angle(R) -> float:
    """angle of a 3 x 3 rotation in radians (atan2 of the antisymmetric part and the trace: accurate near 0)"""
    R = np.asarray(R, np.float64)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(math.atan2(0.5 * np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)))


def register(est, ref, radius: float, T0=None, ref_normals=None, max_iterations: int = 50, schedule=None, method: str = "plane",
             tol_translation: float = 1e-6, tol_rotation: float = 1e-6, trace: bool = False) -> dict:
    """Rigid registration of `est` onto `ref` from the start T0 (4 x 4, est -> ref; identity when None): no scale, no global search (register_global finds a start).
    method "plane": point-to-plane, needs ref_normals ((n, 3) array, or the column of ref where the normals start); "point":
    point-to-point, normals are not used.  Every iteration pairs each est point with its nearest ref point within the radius
    (exactly nearest(ref, est, radius, T)), sums the Gauss-Newton system on the GPU, solves it here (solve_step) and applies
    T <- [exp(w) | t] T (update_se3).  schedule: the radii to run in turn, coarse to fine (default: [radius]); each runs until its step is
    below tol_translation (m) and tol_rotation (rad) -- 1e-6: ten times the fp32 resolution of the transform the device applies, below
    which steps are rounding -- or for max_iterations.  A system outside solve_step's domain ends the loop.
    Returns {"T", "iterations", "inliers", "inlier_share", "rmse", "converged", "reason", "radius", "method", "trace"}: inliers / rmse are
    those of the returned T at the last radius (rmse = sqrt(sum r^2 / inliers): point-to-plane distances for "plane"); converged is True
    only when the last radius met the stop rule; trace (trace=True) lists per iteration {"radius", "T" (before the step), "sys29", "x",
    "inliers", "rmse"}."""
    if method not in ("plane", "point"):
        raise ValueError('method must be "plane" or "point"')
    if method == "plane" and ref_normals is None:
        raise ValueError("point-to-plane registration needs the reference's normals (ref_normals; a PLY without nx / ny / nz has none): "
                         'give them, or use method="point"')
    radii = [float(r) for r in (schedule if schedule is not None else [radius])]
    if not radii:
        raise ValueError("the radius schedule is empty")
    q = _device_points(est)
    nq = int(q.shape[0])
    T = np.eye(4) if T0 is None else np.array(T0, np.float64).reshape(4, 4)
    normals = ref_normals if method == "plane" else None
    tr, iters, converged, reason = [], 0, False, None
    reg = None
    for stage, r in enumerate(radii):
        reg = Registration(ref, r, normals, nq)
        converged = False
        for _ in range(int(max_iterations)):
            s = reg.step(q, T)
            x, why = solve_step(s)
            if trace:
                tr.append({"radius": r, "T": T.copy(), "sys29": s, "x": None if x is None else x.copy(), "inliers": int(s[28]),
                           "rmse": math.sqrt(s[27] / s[28]) if s[28] > 0 else None})
            if x is None:
                reason = why
                break
            T = update_se3(T, x)
            iters += 1
            if float(np.linalg.norm(x[:3])) < tol_translation and float(np.linalg.norm(x[3:])) < tol_rotation:
                converged = True
                break
        if reason is not None:
            break
        if not converged and stage == len(radii) - 1:
            reason = f"no step below the tolerances within {int(max_iterations)} iterations at radius {r:g}"
    s = reg.step(q, T)
    n = int(s[28])
    return {"T": T, "iterations": iters, "inliers": n, "inlier_share": (n / nq if nq else 0.0), "rmse": math.sqrt(s[27] / n) if n else None,
            "converged": bool(converged and reason is None), "reason": reason, "radius": radii[-1], "method": method, "trace": tr}


def registration_summary(res: dict) -> dict:
    """what the command prints of a register() result"""
    T = res["T"]
    return {"T": [[float(v) for v in row] for row in T], "rotation_rad": rotation_angle(T[:3, :3]), "translation_m": float(np.linalg.norm(T[:3, 3])),
            "iterations": res["iterations"], "inliers": res["inliers"], "inlier_share": res["inlier_share"], "rmse": res["rmse"],
            "converged": res["converged"], "reason": res["reason"], "radius": res["radius"], "method": res["method"]}


def read_transform(path: str) -> np.ndarray:
    """a 4 x 4 rigid transform from a text file: 16 numbers (four rows of four; commas and `#` comments allowed), last row 0 0 0 1"""
    v = []
    with open(path) as f:
        for line in f:
            v += [float(x) for x in line.split("#", 1)[0].replace(",", " ").split()]
    if len(v) != 16:
        raise ValueError(f"{path}: expected 16 numbers (a 4 x 4 matrix), got {len(v)}")
    T = np.array(v, np.float64).reshape(4, 4)
    if not np.isfinite(T).all() or np.abs(T[3] - [0, 0, 0, 1]).max() > 1e-9:
        raise ValueError(f"{path}: not a finite matrix with the last row 0 0 0 1")
    if np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() > 1e-4 or np.linalg.det(T[:3, :3]) < 0:
        raise ValueError(f"{path}: the upper 3 x 3 is not a rotation (registration is rigid, without scale)")
    return T


# ------------------------------------------------------------------------------------------------------------------------------------
# normals
# ------------------------------------------------------------------------------------------------------------------------------------
def estimate_normals(points, radius: float, min_neighbours: int = 5, viewpoint=None):
    """Normals of a cloud from its own radius neighbourhoods (mf_cloud_normals_dev; the definition: include/maskfusion_amd.h).  points:
    (n, >= 3) float32 numpy array or device tensor, x, y, z first; viewpoint: three numbers the normals are turned towards, or None (the
    component of largest magnitude is made positive).  Returns numpy (normals float32 (n, 3), variation float32 (n,), count int32 (n,)):
    the unit eigenvector of the smallest eigenvalue of the neighbourhood's covariance, the surface variation l0 / (l0 + l1 + l2) and the
    number of neighbours within `radius`, the point itself included.  A row is NaN (its count still true) where the point is not finite, has
    fewer than min_neighbours (>= 3) neighbours, or its neighbours lie on a line or in one place."""
    import torch
    from .lib import load
    L = load()
    p = _device_points(points)
    n = int(p.shape[0])
    ws, need = _workspace(L, "mf_cloud_normals_workspace", p.device, n)
    out = torch.empty((max(n, 1), 4), dtype=torch.float32, device=p.device)
    cnt = torch.empty(max(n, 1), dtype=torch.int32, device=p.device)
    v = None if viewpoint is None else np.ascontiguousarray(np.asarray(viewpoint, np.float32).reshape(3))
    rc = L.mf_cloud_normals_dev(p.data_ptr() if n else None, int(p.shape[1]), n, float(radius), int(min_neighbours),
                                v.ctypes.data if v is not None else None, out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), need, _stream_of(p.device))
    _check(rc, "mf_cloud_normals_dev", "radius must be finite and > 0, min_neighbours >= 3, a finite viewpoint, coordinates |x / radius| < 2^30")
    o = out[:n].cpu().numpy()
    return np.ascontiguousarray(o[:, :3]), np.ascontiguousarray(o[:, 3]), cnt[:n].cpu().numpy()


def normal_angles(est_normals, ref_normals, idx, T=None) -> np.ndarray:
    """The numpy part of normal_consistency: for every est point i with a partner idx[i] >= 0 whose two normals are finite, the angle in
    degrees between (the rotation of T applied to) est_normals[i] and ref_normals[idx[i]], folded to [0, 90]: acos |n_e . n_r|, taken as
    atan2(|n_e x n_r|, |n_e . n_r|), which keeps its digits near 0.  The normals need not have unit length."""
    ne = np.asarray(est_normals, np.float64).reshape(-1, 3)
    nr = np.asarray(ref_normals, np.float64).reshape(-1, 3)
    idx = np.asarray(idx, np.int64)
    if T is not None:
        ne = ne @ np.asarray(T, np.float64)[:3, :3].T
    hit = np.flatnonzero(idx >= 0)
    a, b = ne[hit], nr[idx[hit]]
    ok = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    a, b = a[ok], b[ok]
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1))))


def normal_consistency(est, est_normals, ref, ref_normals, radius: float, T=None) -> dict:
    """How well the normals of two clouds agree where the clouds meet: every est point (moved by T, 4 x 4 est -> ref, when given) is paired
    with its nearest ref point within `radius` -- nearest(ref, est, radius, T) -- and the pair's angle is that between their normals, folded
    to [0, 90 degrees] so that the orientation of either does not matter.  Returns {"radius", "count" (est points), "pairs" (with a partner
    and two finite normals), "mean_deg", "median_deg", "below": {"10", "20", "30": the share of the pairs under that many degrees}}."""
    _, idx = nearest(ref, est, radius, T)
    ang = normal_angles(est_normals, ref_normals, idx, T)
    out = {"radius": radius, "count": int(len(idx)), "pairs": int(ang.size)}
    out.update({"mean_deg": float(ang.mean()), "median_deg": float(np.median(ang))} if ang.size else {"mean_deg": None, "median_deg": None})
    out["below"] = {str(d): (float(np.count_nonzero(ang < d)) / ang.size if ang.size else 0.0) for d in (10, 20, 30)}
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# global registration
# ------------------------------------------------------------------------------------------------------------------------------------
FPFH_DIM = 33
MIN_MUTUAL = 30           # register_global: fewer mutual matches than this, and every est -> ref match is a correspondence


def voxel_subsample(points, voxel: float) -> np.ndarray:
    """The indices (int64, ascending) of the first point, lowest index, of every occupied voxel: cells are floor(x / voxel) per axis in
    fp64.  Points that are not finite are left out.  Plain numpy."""
    p = np.asarray(points)[:, :3].astype(np.float64)
    if not (math.isfinite(voxel) and voxel > 0):
        raise ValueError("voxel must be finite and > 0")
    ok = np.flatnonzero(np.isfinite(p).all(1))
    if ok.size == 0:
        return np.zeros(0, np.int64)
    cells = np.floor(p[ok] / float(voxel))
    _, first = np.unique(cells, axis=0, return_index=True)       # return_index: the first occurrence
    return np.sort(ok[first]).astype(np.int64)


def fpfh(points, normals, radius: float):
    """FPFH descriptors of a cloud with normals (mf_cloud_fpfh_dev; the definition: include/maskfusion_amd.h).  points (n, >= 3), normals
    (n, 3): float32 numpy arrays or device tensors.  Returns numpy (fpfh float32 (n, 33), spfh int32 (n, 34): the 33 counts of the point's own
    pair histogram and k, the number of counted pairs).  A row of fpfh is NaN where the point or its normal is not finite, the normal is
    zero, or no neighbour within `radius` has a counted pair."""
    import torch
    from .lib import load
    L = load()
    p, nr_ = _device_points(points), _device_points(normals)
    if nr_.shape[0] != p.shape[0]:
        raise ValueError("normals must have one row per point")
    rec = torch.cat([p[:, :3], nr_[:, :3]], 1).contiguous()
    n = int(rec.shape[0])
    ws, need = _workspace(L, "mf_cloud_fpfh_workspace", rec.device, n)
    out = torch.empty((max(n, 1), FPFH_DIM), dtype=torch.float32, device=rec.device)
    cnt = torch.empty((max(n, 1), FPFH_DIM + 1), dtype=torch.int32, device=rec.device)
    rc = L.mf_cloud_fpfh_dev(rec.data_ptr() if n else None, 6, 3, n, float(radius), out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), need,
                             _stream_of(rec.device))
    _check(rc, "mf_cloud_fpfh_dev", "radius must be finite and > 0, coordinates |x / radius| < 2^30")
    return out[:n].cpu().numpy(), cnt[:n].cpu().numpy()


def match_features(target, query):
    """For every query descriptor the nearest target descriptor by brute force (mf_feature_match_dev): (n, dim <= 64) float32 numpy arrays
    or device tensors.  Returns numpy (idx int32, -1: none; d2 float32, the squared distance, +inf: none).  Ties go to the smallest index;
    a row with a NaN matches nothing and is nobody's match."""
    import torch
    from .lib import load
    L = load()
    t, q = (_device_points(a, 0, "descriptors must be (n, dim) float32") for a in (target, query))
    if t.shape[1] != q.shape[1]:
        raise ValueError(f"target descriptors have {t.shape[1]} values, query descriptors {q.shape[1]}")
    nt, nq = int(t.shape[0]), int(q.shape[0])
    idx = torch.empty(max(nq, 1), dtype=torch.int32, device=q.device)
    d2 = torch.empty(max(nq, 1), dtype=torch.float32, device=q.device)
    rc = L.mf_feature_match_dev(t.data_ptr() if nt else None, nt, q.data_ptr() if nq else None, nq, int(q.shape[1]), idx.data_ptr(),
                                d2.data_ptr(), _stream_of(q.device))
    _check(rc, "mf_feature_match_dev", "1 to 64 values per descriptor")
    return idx[:nq].cpu().numpy(), d2[:nq].cpu().numpy()


def _horn_batch(src, dst):
    """align_horn's rule on a batch: src, dst (K, m, 3) fp64 -> R (K, 3, 3), t (K, 3)"""
    ms, md = src.mean(1), dst.mean(1)
    H = np.einsum("kia,kib->kab", src - ms[:, None], dst - md[:, None])
    U, _, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, 1, 2)
    Ut = np.swapaxes(U, 1, 2)
    D = np.ones((len(H), 3))
    D[:, 2] = np.where(np.linalg.det(V @ Ut) < 0, -1.0, 1.0)
    R = (V * D[:, None, :]) @ Ut
    return R, md - np.einsum("kab,kb->ka", R, ms)


def _pose_ransac_device(src, dst, tri, inlier_distance: float, edge_tolerance: float):
    """mf_pose_ransac_dev on (m, 3) float32 correspondences and (h, 3) int32 triples.  Returns numpy (status uint8 (h,), counts uint32 (h,),
    best int32 (2,): index or -1 and count, inlier mask bool (m,), pose fp64 3 x 4 [R | t] or None without a tested triple)."""
    import torch
    from .lib import load
    L = load()
    s, d = _device_points(src), _device_points(dst)
    m, h = int(s.shape[0]), int(len(tri))
    dev = s.device
    t = torch.as_tensor(np.ascontiguousarray(tri, np.int32)).to(dev)
    counts = torch.zeros(max(h, 1), dtype=torch.int32, device=dev)
    status = torch.zeros(max(h, 1), dtype=torch.uint8, device=dev)
    best = torch.zeros(2, dtype=torch.int32, device=dev)
    mask = torch.zeros(max(m, 1), dtype=torch.uint8, device=dev)
    pose = torch.zeros(12, dtype=torch.float64, device=dev)
    rc = L.mf_pose_ransac_dev(s.data_ptr() if m else None, d.data_ptr() if m else None, int(s.shape[1]), m, t.data_ptr() if h else None, h,
                              float(inlier_distance), float(edge_tolerance), counts.data_ptr(), status.data_ptr(), best.data_ptr(),
                              mask.data_ptr(), pose.data_ptr(), _stream_of(dev))
    _check(rc, "mf_pose_ransac_dev", "inlier_distance must be finite and > 0, edge_tolerance in [0, 1), at most 2^24 correspondences and triples")
    b = best.cpu().numpy()               # (the copy waits for the stream)
    return (status[:h].cpu().numpy(), counts[:h].cpu().numpy().view(np.uint32), b, mask[:m].cpu().numpy().astype(bool),
            pose.cpu().numpy().reshape(3, 4) if b[0] >= 0 else None)


def ransac_correspondences(src, dst, inlier_distance: float, hypotheses: int = 20000, seed: int = 0, edge_tolerance: float = 0.1,
                           chunk: int = 512, device: bool = False) -> dict:
    """The hypothesis search of register_global over correspondences src[k] <-> dst[k] ((m, 3) each; the T sought maps src onto dst).
    `hypotheses` triples of three different correspondences are drawn at once from numpy.random.default_rng(seed); a triple is dropped
    when one of its three edges has lengths in src and dst that disagree by more than edge_tolerance (the shorter below 1 - edge_tolerance
    of the longer) -- a rigid motion keeps lengths.  Every other triple is solved by align_horn's rule, in batches, and scored by the
    number of correspondences with |T src - dst| <= inlier_distance, in fp64.  The largest count wins, ties go to the hypothesis drawn
    earlier; T is then fitted again to the winner's inliers (align_horn).  Returns {"T" 4 x 4, "inliers": the winner's count, "inlier_mask"
    bool (m,): under the winning triple's pose, "hypotheses": drawn, "tested": solved and scored}; without a testable triple T is None and
    inliers 0.  The same input and seed give the same result.
    device=True: the same draw of triples, checked, fitted and scored on the GPU (mf_pose_ransac_dev, on the fp32 values of src and dst).
    The edge rule is the same; a triple's pose is the closed form of the header, not align_horn's, so counts and winner may differ from the
    host's.  T is align_horn on the device's inlier mask when that has at least three members, the device's pose otherwise; "tested" counts
    the triples of status 0."""
    src, dst = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    m = len(src)
    out = {"T": None, "inliers": 0, "inlier_mask": np.zeros(m, bool), "hypotheses": int(hypotheses), "tested": 0}
    if m < 3 or len(dst) != m or hypotheses < 1:
        return out
    rng = np.random.default_rng(seed)
    tri = rng.integers(0, m, (int(hypotheses), 3))
    if device:
        status, _, best, mask, pose = _pose_ransac_device(src.astype(np.float32), dst.astype(np.float32), tri, inlier_distance, edge_tolerance)
        out["tested"] = int((status == 0).sum())
        if best[0] < 0:
            return out
        T = np.eye(4)
        T[:3] = pose
        if mask.sum() >= 3:
            T = align_horn(src[mask], dst[mask])
        out.update({"T": T, "inliers": int(best[1]), "inlier_mask": mask})
        return out
    keep = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
    for a, b in ((0, 1), (0, 2), (1, 2)):
        ls = np.linalg.norm(src[tri[:, a]] - src[tri[:, b]], axis=1)
        ld = np.linalg.norm(dst[tri[:, a]] - dst[tri[:, b]], axis=1)
        with np.errstate(invalid="ignore"):
            keep &= np.minimum(ls, ld) >= (1.0 - edge_tolerance) * np.maximum(ls, ld)
            keep &= np.minimum(ls, ld) > 0
    tri = tri[keep]
    out["tested"] = int(len(tri))
    best, best_R, best_t = 0, None, None
    for a in range(0, len(tri), chunk):
        t3 = tri[a:a + chunk]
        R, t = _horn_batch(src[t3], dst[t3])
        moved = np.einsum("kab,mb->kma", R, src) + t[:, None, :]
        cnt = (np.linalg.norm(moved - dst[None], axis=2) <= inlier_distance).sum(1)
        k = int(np.argmax(cnt))                 # the first of equal counts
        if cnt[k] > best:
            best, best_R, best_t = int(cnt[k]), R[k], t[k]
    if best_R is None:
        return out
    mask = np.linalg.norm(src @ best_R.T + best_t - dst, axis=1) <= inlier_distance
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = best_R, best_t
    if mask.sum() >= 3:
        T = align_horn(src[mask], dst[mask])
    out.update({"T": T, "inliers": best, "inlier_mask": mask})
    return out


def _towards_centroid(points, normals):
    """the normals turned to face the centroid of the finite points: a rule that moves with the cloud, which the descriptors need"""
    p, n = np.asarray(points, np.float64), np.asarray(normals, np.float64)
    c = p[np.isfinite(p).all(1)].mean(0) if np.isfinite(p).all(1).any() else np.zeros(3)
    with np.errstate(invalid="ignore"):
        flip = ((c - p) * n).sum(1) < 0
    return np.where(flip[:, None], -n, n).astype(np.float32)


def register_global(est, ref, voxel: float, est_normals=None, ref_normals=None, seed: int = 0, hypotheses: int = 20000,
                    inlier_distance=None, refine: bool = True, min_mutual: int = MIN_MUTUAL, max_iterations: int = 50, method: str = "plane",
                    schedule=None, ransac: str = "host") -> dict:
    """Rigid registration of `est` onto `ref` (numpy (n, 3) float32) WITHOUT a start: a coarse pose from matched FPFH descriptors, then
    register().
      1. both clouds are subsampled to one point per voxel (voxel_subsample);
      2. a cloud without normals gets them from estimate_normals on the whole cloud at radius 2 voxel; for the descriptors the key points'
         normals, given or estimated, are turned to face their cloud's centroid -- an orientation rule that moves with the cloud, which a
         rule of the coordinate axes does not;
      3. FPFH of the key points at radius 5 voxel (fpfh);
      4. descriptors are matched both ways (match_features); the mutual matches are the correspondences, or, with fewer than min_mutual
         of them, every est -> ref match;
      5. ransac_correspondences(seed, hypotheses, inlier_distance -- default 1.5 voxel); ransac="device" runs its search on the GPU
         (device=True: mf_pose_ransac_dev), "host" in numpy;
      6. refine: register() on the FULL clouds from that pose, radii halving from inlier_distance down to voxel / 2, or `schedule`
         (point-to-plane on ref_normals, given or estimated; method "point": point-to-point).
    Returns register()'s dictionary -- with refine=False: T = the coarse pose, iterations 0, converged False, reason "not refined" --
    plus "coarse": {"T", "correspondences", "mutual", "inliers", "hypotheses", "tested", "key_points": [est, ref]}.  Without a coarse pose
    (fewer than three correspondences, no triple passes the edge test) T is the identity, converged False and reason says so.  With the same
    seed the coarse stage is deterministic up to FPFH's last bits (mf_cloud_fpfh_dev sums in the order of its grid's atomics): a
    descriptor distance that ties to fp32 rounding could change a match between two calls."""
    if not (math.isfinite(voxel) and voxel > 0):
        raise ValueError("voxel must be finite and > 0")
    inlier_distance = 1.5 * voxel if inlier_distance is None else float(inlier_distance)
    if not (math.isfinite(inlier_distance) and inlier_distance > 0):
        raise ValueError("inlier_distance must be finite and > 0")
    if ransac not in ("host", "device"):
        raise ValueError('ransac must be "host" or "device"')
    clouds = []
    for pts, nrm in ((est, est_normals), (ref, ref_normals)):
        pts = np.ascontiguousarray(np.asarray(pts, np.float32)[:, :3])
        if nrm is None:
            nrm = estimate_normals(pts, 2.0 * voxel)[0]
        nrm = np.ascontiguousarray(np.asarray(nrm, np.float32)[:, :3])
        if len(nrm) != len(pts):
            raise ValueError("normals must have one row per point")
        key = voxel_subsample(pts, voxel)
        kp = pts[key]
        desc = fpfh(kp, _towards_centroid(kp, nrm[key]), 5.0 * voxel)[0]
        clouds.append((pts, nrm, kp, desc))
    (pe, ne, ke, de), (pr, nr_, kr, dr) = clouds
    e2r = match_features(dr, de)[0]
    r2e = match_features(de, dr)[0]
    hit = np.flatnonzero(e2r >= 0)
    mutual = hit[r2e[e2r[hit]] == hit]
    use = mutual if len(mutual) >= min_mutual else hit
    rs = ransac_correspondences(ke[use], kr[e2r[use]], inlier_distance, hypotheses, seed, device=ransac == "device")
    coarse = {"T": rs["T"], "correspondences": int(len(use)), "mutual": int(len(mutual)), "inliers": rs["inliers"], "hypotheses": rs["hypotheses"],
              "tested": rs["tested"], "key_points": [int(len(ke)), int(len(kr))]}
    if rs["T"] is None:
        res = {"T": np.eye(4), "iterations": 0, "inliers": 0, "inlier_share": 0.0, "rmse": None, "converged": False,
               "reason": f"no coarse pose: {len(use)} correspondences, {rs['tested']} of {rs['hypotheses']} triples passed the edge test",
               "radius": inlier_distance, "method": method, "trace": []}
    elif refine:
        radii = [inlier_distance]
        while radii[-1] / 2.0 > voxel / 2.0:
            radii.append(radii[-1] / 2.0)
        radii.append(voxel / 2.0)
        if schedule is not None:
            radii = [float(r) for r in schedule]
        res = register(pe, pr, radii[-1], T0=rs["T"], ref_normals=nr_ if method == "plane" else None, max_iterations=max_iterations,
                       schedule=radii, method=method)
    else:
        res = {"T": rs["T"], "iterations": 0, "inliers": rs["inliers"], "inlier_share": rs["inliers"] / max(len(use), 1), "rmse": None,
               "converged": False, "reason": "not refined", "radius": inlier_distance, "method": method, "trace": []}
    res["coarse"] = coarse
    return res


def coarse_summary(coarse: dict) -> dict:
    """what the command prints of register_global's coarse block"""
    T = coarse["T"]
    return {"T": None if T is None else [[float(v) for v in row] for row in T], "correspondences": coarse["correspondences"],
            "mutual": coarse["mutual"], "inliers": coarse["inliers"], "hypotheses": coarse["hypotheses"], "tested": coarse["tested"],
            "key_points": coarse["key_points"]}


# ------------------------------------------------------------------------------------------------------------------------------------
# segmentation
# ------------------------------------------------------------------------------------------------------------------------------------
VOID = 255               # a look-up table entry: the raw value belongs to no class
MAX_CLASSES = 64          # classes per side of the device calls (mf_label_confusion_dev)
MAX_RADIUS = 16           # mf_label_boundary_dev


def _device_labels(a):
    """uint8 (n_frames, H, W) on the library's device; a single (H, W) image becomes one frame"""
    import torch
    from .lib import torch_device
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.uint8)))
    if t.dim() == 2:
        t = t[None]
    if t.dtype != torch.uint8 or t.dim() != 3 or t.numel() == 0:
        raise ValueError("labels must be uint8 of shape (n_frames, H, W) or (H, W), not empty")
    return t.to(torch_device()).contiguous()


def _lut_arg(lut, n):
    lut = np.ascontiguousarray(np.asarray(lut, np.uint8).reshape(-1))
    if lut.size != 256:
        raise ValueError("a look-up table has 256 entries")
    if n is None:
        used = lut[lut != VOID]
        n = int(used.max()) + 1 if used.size else 1
    return lut, int(n)


def _label_call(est, gt, lut_est, lut_gt, n_est, n_gt):
    from .lib import load
    e, g = _device_labels(est), _device_labels(gt)
    if e.shape != g.shape:
        raise ValueError(f"estimate {tuple(e.shape)} and ground truth {tuple(g.shape)} differ in shape")
    le, n_est = _lut_arg(lut_est, n_est)
    lg, n_gt = _lut_arg(lut_gt, n_gt)
    return load(), e, g, le, n_est, lg, n_gt, _stream_of(e.device)


def label_confusion_dev(est, gt, lut_est, lut_gt, n_est=None, n_gt=None):
    """label_confusion() with the result left on the device: an int32 tensor (n_frames, n_gt, n_est) holding the uint32 counts"""
    import torch
    L, e, g, le, n_est, lg, n_gt, stream = _label_call(est, gt, lut_est, lut_gt, n_est, n_gt)
    out = torch.empty((e.shape[0], n_gt, n_est), dtype=torch.int32, device=e.device)
    rc = L.mf_label_confusion_dev(e.data_ptr(), g.data_ptr(), int(e.shape[0]), int(e.shape[1]), int(e.shape[2]), le.ctypes.data, n_est,
                                  lg.ctypes.data, n_gt, out.data_ptr(), stream)
    _check(rc, "mf_label_confusion_dev", "1..64 classes per side; table entries below the class count, or 255")
    return out


def label_confusion(est, gt, lut_est, lut_gt, n_est=None, n_gt=None) -> np.ndarray:
    """Region counts of two label streams (mf_label_confusion_dev): est, gt uint8 (n_frames, H, W) numpy arrays or device tensors; lut_est,
    lut_gt 256 entries, raw value -> class index or 255 (void); n_est, n_gt: the class counts (default: the largest index in the table + 1).
    Returns uint32 (n_frames, n_gt, n_est): [f, g, e] = the pixels of frame f with ground truth g and estimate e, void pixels left out."""
    return label_confusion_dev(est, gt, lut_est, lut_gt, n_est, n_gt).cpu().numpy().view(np.uint32)


def label_boundary(est, gt, lut_est, lut_gt, pair, radius: int, n_est=None, n_gt=None) -> np.ndarray:
    """Boundary counts of two label streams (mf_label_boundary_dev; the definitions: include/maskfusion_amd.h).  pair: one entry per
    ground-truth class, the estimate class matched to it or 255; its length is n_gt unless n_gt is given.  radius: 0..16 pixels.
    Returns uint32 (n_frames, n_gt, 4) = n_est_boundary, est_hit, n_gt_boundary, gt_hit."""
    import torch
    pr = np.ascontiguousarray(np.asarray(pair, np.uint8).reshape(-1))
    L, e, g, le, n_est, lg, n_gt, stream = _label_call(est, gt, lut_est, lut_gt, n_est, len(pr) if n_gt is None else n_gt)
    if len(pr) != n_gt:
        raise ValueError(f"pair has {len(pr)} entries for {n_gt} ground-truth classes")
    out = torch.empty((e.shape[0], n_gt, 4), dtype=torch.int32, device=e.device)
    rc = L.mf_label_boundary_dev(e.data_ptr(), g.data_ptr(), int(e.shape[0]), int(e.shape[1]), int(e.shape[2]), le.ctypes.data, n_est,
                                 lg.ctypes.data, n_gt, pr.ctypes.data, int(radius), out.data_ptr(), stream)
    _check(rc, "mf_label_boundary_dev", "1..64 classes per side; table and pair entries below the class count, or 255; radius 0..16")
    return out.cpu().numpy().view(np.uint32)


def build_lut(present, void=None, also_background=()):
    """The look-up table of one side: the distinct raw values that occur (`present`: the values, or 256 flags / counts by value), in ascending
    order, are the classes, with raw 0 -> class 0 whether it occurs or not; `void` (a raw value, or None) -> 255; the raw values in
    also_background -> class 0.  Raw values that do not occur map to 255.  Returns (lut uint8 [256], ids): ids[k] = the raw value of class k.
    More than 64 classes: ValueError."""
    p = np.asarray(present)
    flags = np.zeros(256, bool)
    if p.shape == (256,) and p.dtype != np.uint8:
        flags[:] = p != 0
    else:
        flags[p.astype(np.int64).reshape(-1)] = True
    flags[0] = True
    for v in ([] if void is None else [int(void)]) + [int(v) for v in also_background]:
        if not 0 < v < 256:
            raise ValueError(f"raw value {v}: void and background aliases are raw values 1..255")
        flags[v] = False
    ids = [int(v) for v in np.flatnonzero(flags)]
    if len(ids) > MAX_CLASSES:
        raise ValueError(f"{len(ids)} distinct label values: the segmentation scores handle at most {MAX_CLASSES} per side (background included)")
    lut = np.full(256, VOID, np.uint8)
    lut[ids] = np.arange(len(ids), dtype=np.uint8)
    for v in also_background:
        lut[int(v)] = 0
    return lut, ids


def default_radius(width: int, height: int) -> int:
    """the boundary measure's pixel radius: 0.008 of the image diagonal, at least 1, at most 16 (6 at 640 x 480)"""
    return int(min(MAX_RADIUS, max(1, round(0.008 * math.hypot(width, height)))))


def match_objects(counts) -> np.ndarray:
    """The pairing of seg_metrics: uint8 [n_gt], the estimate class matched to every ground-truth class or 255.  Background (class 0) pairs
    with background; the objects (classes >= 1) are matched one to one so that the sum of their sequence IoUs -- intersections summed over
    the frames by unions summed over the frames -- is largest; a pair without a common pixel is left unmatched."""
    from scipy.optimize import linear_sum_assignment
    c = np.asarray(counts).astype(np.int64).sum(0)
    n_gt, n_est = c.shape
    pair = np.full(n_gt, VOID, np.uint8)
    pair[0] = 0
    if n_gt > 1 and n_est > 1:
        inter = c[1:, 1:]
        union = c.sum(1)[1:, None] + c.sum(0)[None, 1:] - inter
        iou = np.where(union > 0, inter / np.maximum(union, 1), 0.0)
        for r, k in zip(*linear_sum_assignment(iou, maximize=True)):
            if inter[r, k] > 0:
                pair[r + 1] = k + 1
    return pair


def _ratio(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.where(b > 0, a / np.where(b > 0, b, 1.0), 0.0)


def seg_metrics(counts, boundary_fn, gt_ids=None, est_ids=None) -> dict:
    """From counts to scores, without a GPU.  counts: (n_frames, n_gt, n_est) region counts (label_confusion's); boundary_fn(pair) -> the
    (n_frames, n_gt, 4) boundary counts for that pairing (label_boundary's); gt_ids / est_ids: the raw value of every class (build_lut's
    ids; default: the class indices), used to name objects and models.  Class 0 is the background on both sides.

    Returns {"pair", "objects", "summary"}.  pair: match_objects(counts).  objects: one entry per ground-truth class >= 1:
      gt_id, model_id (None: unmatched), iou -- the sequence IoU, intersections over unions both summed over the frames --, and
      J, P, R, F, JF -- the means, over the frames in which the object has at least one counted ground-truth pixel (`frames` of them), of
      the frame's J = intersection / union, P = est_hit / n_est_boundary, R = gt_hit / n_gt_boundary, F = 2 P R / (P + R) and (J + F) / 2.
      A ratio with a zero denominator is 0, F is 0 when P + R = 0, an object seen in no frame has means 0, an unmatched object scores 0.
    summary: objects, matched, the means over the objects of iou, J, P, R, F, JF (None without objects), unmatched_models (the estimate's
    classes >= 1 matched to nothing) and background_iou (the sequence IoU of class 0 with class 0)."""
    c = np.asarray(counts).astype(np.int64)
    if c.ndim != 3:
        raise ValueError("counts must have the shape (n_frames, n_gt, n_est)")
    n_frames, n_gt, n_est = c.shape
    gt_ids = list(range(n_gt)) if gt_ids is None else [int(v) for v in gt_ids]
    est_ids = list(range(n_est)) if est_ids is None else [int(v) for v in est_ids]
    pair = match_objects(c)
    b = np.asarray(boundary_fn(pair)).astype(np.int64)
    if b.shape != (n_frames, n_gt, 4):
        raise ValueError(f"boundary_fn returned the shape {b.shape}, expected {(n_frames, n_gt, 4)}")
    gt_area, est_area = c.sum(2), c.sum(1)               # [f, g], [f, e]
    keys = ("iou", "J", "P", "R", "F", "JF")
    objects = []
    for g in range(1, n_gt):
        o = {"gt_id": gt_ids[g], "model_id": None, "frames": int(np.count_nonzero(gt_area[:, g]))}
        o.update({k: 0.0 for k in keys})
        e = int(pair[g])
        if e != VOID:
            seen = gt_area[:, g] > 0
            inter = c[:, g, e]
            union = gt_area[:, g] + est_area[:, e] - inter
            J = _ratio(inter, union)
            P, R = _ratio(b[:, g, 1], b[:, g, 0]), _ratio(b[:, g, 3], b[:, g, 2])
            F = _ratio(2.0 * P * R, P + R)
            o["model_id"] = est_ids[e]
            o["iou"] = float(_ratio(inter.sum(), union.sum()))
            if seen.any():
                for k, v in (("J", J), ("P", P), ("R", R), ("F", F), ("JF", 0.5 * (J + F))):
                    o[k] = float(v[seen].mean())
        objects.append(o)
    matched = {int(e) for e in pair[1:] if e != VOID}
    bg_inter = c[:, 0, 0].sum()
    summary = {"objects": len(objects), "matched": len(matched), "frames": int(n_frames)}
    for k in keys:
        summary[k] = float(np.mean([o[k] for o in objects])) if objects else None
    summary["unmatched_models"] = [est_ids[e] for e in range(1, n_est) if e not in matched]
    summary["background_iou"] = float(_ratio(bg_inter, gt_area[:, 0].sum() + est_area[:, 0].sum() - bg_inter))
    return {"pair": pair, "objects": objects, "summary": summary}


class SegmentationScorer:
    """Collects the frames of a run, estimate and ground truth, on the device and scores them there.  add() takes label images from the
    host or the device, add_from() takes the estimate from a live context's label image without a download.  Alongside the frames the
    scorer keeps, on the device, how often every raw value occurred on either side: result() builds the look-up tables from that
    (build_lut), counts regions (mf_label_confusion_dev), matches the objects (match_objects), counts boundaries for that pairing
    (mf_label_boundary_dev) and returns seg_metrics' scores.

    void: a raw ground-truth value that marks pixels to leave out (None: no such value).  The estimate's value 255 -- "ignored" in the
    context's label image, written as 0 by the -es export -- counts as background."""

    EST_IGNORED = 255

    def __init__(self, void=None):
        self.void = void
        self._est, self._gt, self._hist = [], [], []
        self.shape = None

    # a 256-bin histogram of raw values from the region kernel itself: class (v >> 6, v & 63) of a stream compared with itself
    _LO = (np.arange(256) & 63).astype(np.uint8)
    _HI = (np.arange(256) >> 6).astype(np.uint8)

    def _raw_counts(self, t):
        return label_confusion_dev(t, t, self._LO, self._HI, 64, 4).sum(0)

    @staticmethod
    def _own(a):
        """device labels that nobody else writes: a copy, unless moving `a` to the device already made one"""
        t = _device_labels(a)
        shared = a.data_ptr() == t.data_ptr() if hasattr(a, "data_ptr") else t.device.type == "cpu"
        return t.clone() if shared else t

    def _add(self, e, g):
        if e.shape != g.shape:
            raise ValueError(f"estimate {tuple(e.shape)} and ground truth {tuple(g.shape)} differ in shape")
        if self.shape is None:
            self.shape = tuple(e.shape[1:])
        if tuple(e.shape[1:]) != self.shape:
            raise ValueError(f"frames of {tuple(e.shape[1:])} added to a scorer of {self.shape} frames")
        self._est.append(e)
        self._gt.append(g)
        self._hist.append((self._raw_counts(e), self._raw_counts(g)))

    def add(self, est, gt):
        """one frame (H, W) or a batch (n, H, W) of both sides, numpy arrays or device tensors; the scorer keeps device copies"""
        self._add(self._own(est), self._own(gt))

    def add_from(self, mf, gt):
        """the frame `mf` (a MaskFusion context) processed last against its ground truth (H, W): the estimate is the context's label image,
        copied device to device (mf_export_segmentation_dev)"""
        import torch
        from .lib import torch_device
        e = torch.empty((1, mf.height, mf.width), dtype=torch.uint8, device=torch_device())
        mf._chk(mf._L.mf_export_segmentation_dev(mf._h, e.data_ptr()))
        mf.sync()               # the copy runs on the context's stream, what follows on torch's
        self._add(e, self._own(gt))

    @property
    def frames(self) -> int:
        return sum(int(t.shape[0]) for t in self._est)

    def tables(self):
        """((lut_est, est_ids), (lut_gt, gt_ids)) for the frames added so far"""
        if not self._est:
            raise ValueError("no frames were added")
        he = sum(h[0] for h in self._hist).cpu().numpy().reshape(256)
        hg = sum(h[1] for h in self._hist).cpu().numpy().reshape(256)
        alias = (self.EST_IGNORED,) if he[self.EST_IGNORED] else ()
        return build_lut(he, also_background=alias), build_lut(hg, void=self.void)

    def stacked(self):
        """(est, gt) as two device tensors (n_frames, H, W)"""
        import torch
        if len(self._est) > 1:
            self._est, self._gt = [torch.cat(self._est)], [torch.cat(self._gt)]
        return self._est[0], self._gt[0]

    def result(self, radius=None) -> dict:
        """seg_metrics of everything added, with "radius" in the summary and the region counts (n_frames, n_gt, n_est) under "counts";
        radius None: default_radius of the frame size"""
        (le, est_ids), (lg, gt_ids) = self.tables()
        est, gt = self.stacked()
        r = default_radius(self.shape[1], self.shape[0]) if radius is None else int(radius)
        if not 0 <= r <= MAX_RADIUS:
            raise ValueError(f"radius {r}: the boundary measure takes 0..{MAX_RADIUS} pixels")
        counts = label_confusion(est, gt, le, lg, len(est_ids), len(gt_ids))
        res = seg_metrics(counts, lambda pair: label_boundary(est, gt, le, lg, pair, r, len(est_ids), len(gt_ids)), gt_ids, est_ids)
        res["summary"]["radius"] = r
        res["counts"] = counts
        return res


def read_segmentation_run(est_dir: str, gt_dir: str, prefix: str = "Mask", index_width: int = 4):
    """The label images a run wrote with -es and the ground-truth masks of its sequence: (est, gt, ticks), est and gt uint8 (n, H, W).
    est_dir holds Segmentation<tick>.png (model id per pixel, 0: background or ignored); gt_dir holds <prefix>####.png / .pgm id images,
    found and loaded as the image-directory reader does (io.readers.mask_files, load_mask).  The frame processed at tick t is the reader's
    frame t - 1: mask file index t - 1 + startIndex.  ValueError naming the file for a segmentation image without its mask file or of
    another size."""
    from .io.readers import load_mask, mask_files
    ticks = sorted(int(m.group(1)) for m in (re.fullmatch(r"Segmentation(\d+)\.png", fn) for fn in os.listdir(est_dir)) if m)
    if not ticks:
        raise ValueError(f"{est_dir} holds no Segmentation<tick>.png (the -es export)")
    ext, start = mask_files(gt_dir, prefix, index_width)
    est, gt = [], []
    for t in ticks:
        ep = os.path.join(est_dir, f"Segmentation{t}.png")
        gp = os.path.join(gt_dir, f"{prefix}{t - 1 + start:0{index_width}d}{ext}")
        if not os.path.exists(gp):
            raise ValueError(f"{ep}: its mask file {gp} does not exist (tick t pairs with mask index t - 1 + {start})")
        e, g = load_mask(ep), load_mask(gp)
        if e.shape != g.shape:
            raise ValueError(f"{ep} has {e.shape[1]} x {e.shape[0]} pixels, its mask file {gp} {g.shape[1]} x {g.shape[0]}")
        if est and e.shape != est[0].shape:
            raise ValueError(f"{ep} has {e.shape[1]} x {e.shape[0]} pixels, the images before it {est[0].shape[1]} x {est[0].shape[0]}")
        est.append(e)
        gt.append(g)
    return np.stack(est), np.stack(gt), ticks


def score_segmentation(est_dir: str, gt_dir: str, prefix: str = "Mask", index_width: int = 4, radius=None, void=None) -> list:
    """what the command prints for --seg-gt: one dict per ground-truth object and the summary last"""
    est, gt, ticks = read_segmentation_run(est_dir, gt_dir, prefix, index_width)
    sc = SegmentationScorer(void=void)
    sc.add(est, gt)
    res = sc.result(radius)
    out = [dict(segmentation_object=o.pop("gt_id"), **o) for o in (dict(o) for o in res["objects"])]
    out.append({"segmentation": dict(res["summary"], first_tick=ticks[0], last_tick=ticks[-1])})
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# views: the map's render against the input frame
# ------------------------------------------------------------------------------------------------------------------------------------
VIEW_GROUPS = 64          # groups per call of mf_view_score_dev
VIEW_COUNTERS = 10
VIEW_FIX = float(1 << 24)   # the fixed point of counters 5 and 9
VIEW_KEYS = ("coverage", "depth_coverage", "depth_l1", "depth_within_tau", "psnr", "psnr_covered", "ssim")
_FLT_MAX = float(np.finfo(np.float32).max)


def _device_frames(a, dtype, channels, what):
    """(n_frames, H, W[, channels]) of `dtype` on the library's device; a single image becomes one frame"""
    import torch
    from .lib import torch_device
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype)))
    want = 3 + (channels > 0)
    if t.dim() == want - 1:
        t = t[None]
    if t.dtype != torch.as_tensor(np.zeros(0, dtype)).dtype or t.dim() != want or t.numel() == 0 or (channels and t.shape[-1] != channels):
        raise ValueError(f"{what} must be {np.dtype(dtype).name} of shape (n_frames, H, W{', %d' % channels if channels else ''}), not empty")
    return t.to(torch_device()).contiguous()


def _view_call(r, rd, c, d, g, n_groups, max_depth, tau, stream):
    """mf_view_score_dev on device tensors that are already in shape -> the counters as an int64 tensor (n_frames, n_groups, 10)"""
    import torch
    from .lib import load
    shape = tuple(rd.shape)
    if tuple(r.shape) != shape + (4,) or tuple(c.shape) != shape + (3,) or tuple(d.shape) != shape or (g is not None and tuple(g.shape) != shape):
        raise ValueError(f"render {tuple(r.shape)} / {tuple(rd.shape)}, frame {tuple(c.shape)} / {tuple(d.shape)}"
                         + (f", groups {tuple(g.shape)}" if g is not None else "") + ": the shapes do not belong together")
    out = torch.empty((shape[0], int(n_groups), VIEW_COUNTERS), dtype=torch.int64, device=rd.device)
    md = min(float(max_depth), _FLT_MAX)          # "no limit" is FLT_MAX
    rc = load().mf_view_score_dev(r.data_ptr(), rd.data_ptr(), c.data_ptr(), d.data_ptr(), g.data_ptr() if g is not None else None, shape[0], shape[1],
                                  shape[2], int(n_groups), md, float(tau), out.data_ptr(), stream)
    _check(rc, "mf_view_score_dev", "1..64 groups, at most 2^24 pixels per frame, max_depth > 0, tau >= 0 and finite")
    return out


def view_counts(render_rgba, render_depth, rgb, depth, group=None, n_groups=1, max_depth=math.inf, tau=0.01) -> np.ndarray:
    """The counters behind the view scores (mf_view_score_dev; the definitions: include/maskfusion_amd.h): a render of the map -- render_rgba
    uint8 (n_frames, H, W, 4), render_depth float32 (n_frames, H, W), 0 where nothing was drawn -- against the frames the camera saw -- rgb
    uint8 (n_frames, H, W, 3), depth float32 in metres.  group: uint8 per pixel, the group the pixel is counted in (None: all in group 0;
    a value >= n_groups: nowhere).  Inputs are numpy arrays or device tensors; a single image is one frame.
    Returns uint64 (n_frames, n_groups, 10); counter 9 is a two's-complement int64."""
    r, rd = _device_frames(render_rgba, np.uint8, 4, "render_rgba"), _device_frames(render_depth, np.float32, 0, "render_depth")
    c, d = _device_frames(rgb, np.uint8, 3, "rgb"), _device_frames(depth, np.float32, 0, "depth")
    g = None if group is None else _device_frames(group, np.uint8, 0, "group")
    return _view_call(r, rd, c, d, g, n_groups, max_depth, tau, _stream_of(rd.device)).cpu().numpy().view(np.uint64)


def _view_scores(c) -> dict:
    """the seven scores of one row of ten counters (Python ints); None for a zero denominator or a zero error sum"""
    c = [int(v) for v in c]
    div = lambda a, b: a / b if b else None
    psnr = lambda err, n: 10.0 * math.log10(255.0 * 255.0 * (3 * n) / err) if n and err else None
    return {"coverage": div(c[1], c[0]), "depth_coverage": div(c[3], c[2]), "depth_l1": div(c[5] / VIEW_FIX, c[3]),
            "depth_within_tau": div(c[4], c[3]), "psnr": psnr(c[6], c[0]), "psnr_covered": psnr(c[7], c[1]), "ssim": div(c[9] / VIEW_FIX, c[8])}


def view_metrics(counts) -> dict:
    """From counters to scores, without a GPU.  counts: (n_frames, n_groups, 10), view_counts' result.  Per row of counters:
      coverage = c1 / c0, depth_coverage = c3 / c2, depth_l1 (m) = c5 / 2^24 / c3, depth_within_tau = c4 / c3,
      psnr = 10 log10(255^2 3 c0 / c6), psnr_covered the same from c7 and c1, ssim = c9 / 2^24 / c8;
    None for a zero denominator and, for the two PSNRs, a zero error sum.
    Returns {"frames", "groups", "summary"}.  frames[f][g]: the scores of frame f and group g.  groups[g]: {"group", "pixels", "frames" (those
    in which the group has a pixel), the scores POOLED over the frames (from the counters summed over the frames), and under "mean" the
    mean of each per-frame score over the frames where it is defined (None: nowhere)}.  summary: the same two for all groups together (the
    counters summed over the groups: every pixel that is not void)."""
    c = np.asarray(counts)
    if c.ndim != 3 or c.shape[2] != VIEW_COUNTERS:
        raise ValueError("counts must have the shape (n_frames, n_groups, 10)")
    c = np.ascontiguousarray(c.astype(np.uint64)).view(np.int64).astype(object)      # Python integers: sums over long runs cannot wrap

    def sequence(rows):
        per_frame = [_view_scores(r) for r in rows]
        pooled = _view_scores(rows.sum(0)) if len(rows) else _view_scores([0] * VIEW_COUNTERS)
        mean = {}
        for k in VIEW_KEYS:
            vals = [s[k] for s in per_frame if s[k] is not None]
            mean[k] = float(np.mean(vals)) if vals else None
        return per_frame, dict(pooled, mean=mean)

    n_frames, n_groups = c.shape[:2]
    frames = [[None] * n_groups for _ in range(n_frames)]
    groups = []
    for g in range(n_groups):
        per_frame, scores = sequence(c[:, g])
        for f in range(n_frames):
            frames[f][g] = per_frame[f]
        groups.append(dict(group=g, pixels=int(c[:, g, 0].sum()), frames=int(np.count_nonzero(c[:, g, 0])), **scores))
    _, summary = sequence(c.sum(1))
    return {"frames": frames, "groups": groups, "summary": dict(summary, frames=int(n_frames))}


def _torch_ready():
    """torch's side of the GPU, opened now.  torch brings a HIP runtime of its own, and in a process where the library's context exists
    first that runtime finds no device: whoever uses a live context together with torch opens torch's side BEFORE MaskFusion() -- creating
    the ViewScorer first does it."""
    import torch
    from .lib import MFError, torch_device
    if torch_device() != "cuda" or torch.cuda.is_initialized():
        return
    try:
        torch.cuda.init()
    except RuntimeError as e:
        raise MFError("torch cannot open the GPU once the library's context exists: create the ViewScorer (or call torch.cuda.init()) "
                      "before MaskFusion()") from e


class ViewScorer:
    """Scores the map's renders against the frames of a run (SegmentationScorer's counterpart for view_counts / view_metrics).  add() takes
    the five images of one or more frames; add_from() renders a live context from the camera that just saw the frame and compares on the
    device: nothing is downloaded but the counters, and those in result().

    Create the scorer before the context it will score (see _torch_ready).

    Groups: add() takes them as given.  add_from() counts every pixel under the model that drew it: group 0 is "nothing drawn", a model id
    gets the next free group when it is first seen and keeps it; ids past group 63 are void."""

    def __init__(self, max_depth=math.inf, tau=0.01):
        self.max_depth, self.tau = float(max_depth), float(tau)
        _torch_ready()
        self._counts = []
        self._group_of = {}              # model id -> group
        self._buffers = None
        self._keep = None

    def add(self, render_rgba, render_depth, rgb, depth, group=None):
        """one frame or a batch of the five images, numpy arrays or device tensors (view_counts' arguments; group values 0..63, others void)"""
        r, rd = _device_frames(render_rgba, np.uint8, 4, "render_rgba"), _device_frames(render_depth, np.float32, 0, "render_depth")
        c, d = _device_frames(rgb, np.uint8, 3, "rgb"), _device_frames(depth, np.float32, 0, "depth")
        g = None if group is None else _device_frames(group, np.uint8, 0, "group")
        self._counts.append(_view_call(r, rd, c, d, g, VIEW_GROUPS, self.max_depth, self.tau, _stream_of(rd.device)))

    def _groups_for(self, ids):
        """the group of every model list index, shifted by one: entry 0 is "no model" """
        table = [0]
        for i in ids:
            if i not in self._group_of:
                self._group_of[i] = len(self._group_of) + 1
            table.append(self._group_of[i] if self._group_of[i] < VIEW_GROUPS else VOID)
        return table

    def add_from(self, mf, rgb, depth, view=None):
        """the frame `mf` (a MaskFusion context) processed last, rgb (H, W, 3) uint8 and depth (H, W) float32 in metres, against the render of
        the context's maps from view (default: mf.sensorRenderView()).  Render, group look-up and comparison are enqueued on the
        context's stream; the call does not wait for them."""
        import contextlib
        import torch
        from .lib import torch_device
        if view is None:
            view = mf.sensorRenderView()
        H, W = int(view.height), int(view.width)
        dev = torch_device()
        on_stream = contextlib.nullcontext()
        if dev == "cuda":
            torch.cuda.current_stream().synchronize()          # inputs that torch's stream is still writing
            on_stream = torch.cuda.stream(torch.cuda.ExternalStream(mf.stream()))
        with on_stream:
            c, d = _device_frames(rgb, np.uint8, 3, "rgb"), _device_frames(depth, np.float32, 0, "depth")
            if tuple(d.shape) != (1, H, W):
                raise ValueError(f"a frame of {tuple(d.shape[1:])} against a view of {(H, W)}")
            if self._buffers is None or tuple(self._buffers[1].shape) != (1, H, W):
                self._buffers = (torch.empty((1, H, W, 4), dtype=torch.uint8, device=dev), torch.empty((1, H, W), dtype=torch.float32, device=dev),
                                 torch.empty((1, H, W), dtype=torch.int32, device=dev))
            r, rd, model = self._buffers
            mf.renderViewDevice(view, r.data_ptr(), rd.data_ptr(), model.data_ptr())
            table = torch.as_tensor(self._groups_for(mf.modelIDs()), dtype=torch.uint8).to(dev)
            g = table[(model + 1).long()].contiguous()
            self._counts.append(_view_call(r, rd, c, d, g, VIEW_GROUPS, self.max_depth, self.tau, mf.stream() or None))
        self._keep = (c, d, g)             # alive until the kernel has read them: the next call's view waits for the context's stream

    @property
    def frames(self) -> int:
        return sum(int(t.shape[0]) for t in self._counts)

    def counts(self) -> np.ndarray:
        """uint64 (n_frames, 64, 10) of everything added so far; waits for the device"""
        import torch
        if not self._counts:
            raise ValueError("no frames were added")
        if self._counts[0].device.type == "cuda":
            torch.cuda.synchronize()
        if len(self._counts) > 1:
            self._counts = [torch.cat(self._counts)]
        return self._counts[0].cpu().numpy().view(np.uint64)

    def result(self) -> dict:
        """{"groups", "summary", "frames", "counts"}: view_metrics' groups (pooled scores and "mean") for the groups that were assigned to a
        model or hold a pixel, each with the "model_id" it stands for (None: group 0 of add_from, "nothing drawn", and every group of add());
        view_metrics' summary with tau; the number of frames; the counters (n_frames, 64, 10)"""
        counts = self.counts()
        m = view_metrics(counts)
        id_of = {g: i for i, g in self._group_of.items()}
        groups = [dict(o, model_id=id_of.get(o["group"])) for o in m["groups"] if o["pixels"] or o["group"] in id_of]
        return {"groups": groups, "summary": dict(m["summary"], tau=self.tau), "frames": int(counts.shape[0]), "counts": counts}


# ------------------------------------------------------------------------------------------------------------------------------------
# cloud visibility: which part of a reference the sequence observed
# ------------------------------------------------------------------------------------------------------------------------------------
VISIBILITY_CHUNK = 16     # frames per call of observe_sequence: 20 MB of depth at 640 x 480, never the whole stack
OBSERVED_NEAR = 0.01      # the near plane of the command's frusta (m); what a sensor cannot measure is a hole in its depth already


def cam_from_cloud(cam_to_world, cloud_to_world=None) -> np.ndarray:
    """The (n_frames, 12) float32 array mf_cloud_visibility_dev takes -- the rows of every frame's 3 x 4 from the cloud's frame into the
    camera's -- from 4 x 4 camera -> world poses (one, or a stack) and, when the cloud is not in the world frame, its own frame -> world.
    Inverse and product in fp64, rounded once at the end."""
    T = np.asarray(cam_to_world, np.float64).reshape(-1, 4, 4)
    M = np.linalg.inv(T)
    if cloud_to_world is not None:
        M = M @ np.asarray(cloud_to_world, np.float64).reshape(4, 4)
    return np.ascontiguousarray(M[:, :3, :].reshape(-1, 12).astype(np.float32))


class Visibility:
    """Classifies the points of one cloud against the depth frames of a sequence, chunk of frames by chunk, on the device
    (mf_cloud_visibility_dev; the rule: include/maskfusion_amd.h).  points: (n, >= 3) float32 numpy or a device tensor, x y z first;
    fx, fy, cx, cy: the frames' intrinsics; near, far: the frustum's depth range (far inf: no limit); a point is ON SURFACE in a frame when
    its camera z is within tol_abs + tol_rel * d of the depth d measured at its pixel.  add() uploads a chunk and enqueues; nothing is
    downloaded before result()."""

    def __init__(self, points, fx: float, fy: float, cx: float, cy: float, near: float = OBSERVED_NEAR, far: float = math.inf,
                 tol_abs: float = 0.05, tol_rel: float = 0.0):
        import torch
        self._p = _device_points(points)
        self.intrinsics = (float(fx), float(fy), float(cx), float(cy))
        self.near, self.far, self.tol_abs, self.tol_rel = float(near), float(far), float(tol_abs), float(tol_rel)
        n = int(self._p.shape[0])
        self._counts = torch.empty((max(n, 1), 4), dtype=torch.int32, device=self._p.device)      # uint32 on the device
        self._first = torch.empty(max(n, 1), dtype=torch.int32, device=self._p.device)
        self.frames = 0
        self.shape = None

    def add(self, depth_frames, cam_from_cloud):
        """one chunk: depth float32 (n_frames, H, W) in metres (a single image is one frame) and cam_from_cloud()'s (n_frames, 12)"""
        import torch
        from .lib import load
        d = _device_frames(depth_frames, np.float32, 0, "depth_frames")
        m = cam_from_cloud if isinstance(cam_from_cloud, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(cam_from_cloud, np.float32)))
        if m.dtype != torch.float32 or m.numel() != 12 * int(d.shape[0]):
            raise ValueError(f"{int(d.shape[0])} frames need a float32 cam_from_cloud of shape ({int(d.shape[0])}, 12)")
        if self.shape is not None and tuple(d.shape[1:]) != self.shape:
            raise ValueError(f"frames of {tuple(d.shape[1:])} after frames of {self.shape}")
        m = m.to(d.device).contiguous()
        n = int(self._p.shape[0])
        fx, fy, cx, cy = self.intrinsics
        rc = load().mf_cloud_visibility_dev(self._p.data_ptr() if n else None, int(self._p.shape[1]), n, d.data_ptr(), m.data_ptr(), int(d.shape[0]),
                                            int(d.shape[1]), int(d.shape[2]), fx, fy, cx, cy, self.near, min(self.far, _FLT_MAX), self.tol_abs,
                                            self.tol_rel, self.frames, int(self.frames > 0), self._counts.data_ptr(), self._first.data_ptr(),
                                            _stream_of(d.device))
        _check(rc, "mf_cloud_visibility_dev", "at most 2^30 points and 2^24 pixels per frame, fx and fy finite and not 0, 0 < near < far, "
               "tolerances >= 0 and finite")
        self.shape = tuple(d.shape[1:])
        self.frames += int(d.shape[0])

    def result(self):
        """(counts uint32 (n, 4) = {frames in frustum, on surface, seen through, occluded}, first int32 (n,) = the first frame, counted over all
        add() calls, in which the point was on the surface, or -1) as numpy; waits for the device"""
        n = int(self._p.shape[0])
        if self.frames == 0 or n == 0:
            return np.zeros((n, 4), np.uint32), np.full(n, -1, np.int32)
        return self._counts[:n].cpu().numpy().view(np.uint32), self._first[:n].cpu().numpy()


def observed(counts, rule: str = "seen", min_frames: int = 1) -> np.ndarray:
    """bool per point from Visibility's counts: did the sequence observe the point?
      "seen": on surface + seen through >= min_frames -- the sensor's ray reached the point's depth, whether it found the point there or
              measured something farther;
      "surface": on surface >= min_frames."""
    c = np.asarray(counts).astype(np.int64)
    if c.ndim != 2 or c.shape[1] != 4:
        raise ValueError("counts must have the shape (n, 4)")
    if int(min_frames) < 1:
        raise ValueError("min_frames must be at least 1")
    if rule == "seen":
        k = c[:, 1] + c[:, 2]
    elif rule == "surface":
        k = c[:, 1]
    else:
        raise ValueError(f"rule {rule!r}: 'seen' or 'surface'")
    return k >= int(min_frames)


def visibility_summary(counts, keep, frames=None) -> dict:
    """What became of the points, from Visibility's counts and observed()'s mask: {"frames" (as given), "points", "never_in_frustum",
    "only_holes" (in a frustum, never with a valid depth sample), "occluded_only" (classified, and occluded every time), "reached" (on surface
    or seen through at least once), "on_surface", "seen_through" (each at least once; a point can be both), "kept"}.  The first four counts
    after "points" partition the points."""
    c = np.asarray(counts).astype(np.int64)
    keep = np.asarray(keep)
    if c.ndim != 2 or c.shape[1] != 4 or keep.shape != (len(c),):
        raise ValueError("counts must have the shape (n, 4) and keep one entry per point")
    classified = c[:, 1] + c[:, 2] + c[:, 3]
    reached = (c[:, 1] + c[:, 2]) > 0
    return {"frames": None if frames is None else int(frames), "points": int(len(c)),
            "never_in_frustum": int(np.count_nonzero(c[:, 0] == 0)),
            "only_holes": int(np.count_nonzero((c[:, 0] > 0) & (classified == 0))),
            "occluded_only": int(np.count_nonzero((classified > 0) & ~reached)),
            "reached": int(np.count_nonzero(reached)),
            "on_surface": int(np.count_nonzero(c[:, 1])), "seen_through": int(np.count_nonzero(c[:, 2])),
            "kept": int(np.count_nonzero(keep))}


def observe_sequence(points, log, pose_log, intrinsics, pose_to_cloud=None, tol_abs: float = 0.05, tol_rel: float = 0.0, near: float = OBSERVED_NEAR,
                     max_depth=None, stride: int = 1, time_scale: float = 1e-6, max_dt: float = 0.02, chunk: int = VISIBILITY_CHUNK):
    """Visibility of `points` over a recorded sequence.  log: a sequence directory or a .klg (io.readers.open_log; depth only is used, read
    and uploaded `chunk` frames at a time); pose_log: read_tum()'s (timestamps in seconds, camera -> world poses); pose_to_cloud: 4 x 4 from
    the poses' world into the frame of `points` (None: the same frame); intrinsics: (fx, fy, cx, cy) or load_calibration()'s six values.
    Every stride-th frame is paired with a pose by associate(frame timestamp * time_scale, pose timestamps, max_dt); a frame without a pose
    is skipped.  max_depth: depth samples beyond it are holes and the frusta end there -- with the run's depth cutoff, only what the run was
    allowed to fuse counts as observed.  Returns (counts, first, {"frames_used", "frames_skipped"}); ValueError when no frame has a pose."""
    from .io.readers import open_log
    fx, fy, cx, cy = (float(v) for v in intrinsics[:4])
    size = tuple(intrinsics[4:6]) if len(intrinsics) >= 6 and intrinsics[4] is not None else None
    reader = open_log(log, *(size or ()))
    try:
        stamps = np.asarray(reader.timestamps(), np.float64)
        chosen = np.arange(0, len(stamps), max(1, int(stride)))
        pairs = associate(stamps[chosen] * float(time_scale), pose_log[0], max_dt)
        if len(pairs) == 0:
            raise ValueError(f"none of the {len(chosen)} frames of {log} has a pose within {max_dt} s (frame timestamps are multiplied by {time_scale:g})")
        pose_of = {int(chosen[i]): int(j) for i, j in pairs}
        to_cloud = np.eye(4) if pose_to_cloud is None else np.asarray(pose_to_cloud, np.float64)
        far = math.inf if max_depth is None else float(max_depth)
        vis = Visibility(points, fx, fy, cx, cy, near, far, tol_abs, tol_rel)
        frames = (reader.load(k) for k in sorted(pose_of)) if hasattr(reader, "load") else (f for f in reader if f.index in pose_of)
        depth, poses = [], []

        def flush():
            if depth:
                vis.add(np.stack(depth), cam_from_cloud(np.stack(poses)))
                depth.clear()
                poses.clear()
        for f in frames:
            d = np.asarray(f.depth, np.float32)
            if size is not None and d.shape != (size[1], size[0]):
                raise ValueError(f"the calibration names frames of {size[0]} x {size[1]}, {log} holds {d.shape[1]} x {d.shape[0]}")
            if max_depth is not None:
                d = np.where(d > np.float32(max_depth), np.float32(0), d)
            depth.append(d)
            poses.append(to_cloud @ pose_log[1][pose_of[f.index]])
            if len(depth) == max(1, int(chunk)):
                flush()
        flush()
    finally:
        if hasattr(reader, "close"):
            reader.close()
    counts, first = vis.result()
    return counts, first, {"frames_used": int(vis.frames), "frames_skipped": int(len(chosen) - len(pairs))}


# ------------------------------------------------------------------------------------------------------------------------------------
# the command
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_files(d: str):
    """{id: {"poses": path, "cloud": path}} of a run's export directory"""
    out = {}
    for fn in sorted(os.listdir(d)):
        m = re.fullmatch(r"(poses|cloud)-(\d+)\.(txt|ply)", fn)
        if m and (m.group(1) == "poses") == (m.group(3) == "txt"):
            out.setdefault(int(m.group(2)), {})[m.group(1)] = os.path.join(d, fn)
    return out


def _apply(T, pts):
    return (pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def _object_to_world(est_log, ref_log, max_dt):
    """obj -> world of both runs at the latest timestamp both logs have (associated within max_dt), or None"""
    pairs = associate(est_log[0], ref_log[0], max_dt)
    if len(pairs) == 0:
        return None
    i, j = pairs[np.argmax(est_log[0][pairs[:, 0]])]
    return est_log[1][i], ref_log[1][j], float(est_log[0][i])


def _clean(o):
    if isinstance(o, float):
        return o if math.isfinite(o) else None
    if isinstance(o, dict):
        return {k: _clean(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_clean(v) for v in o]
    return o


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m maskfusion_amd.eval", description=__doc__.split("\n\n")[0])
    ap.add_argument("--est", required=True, help="export directory of the run to evaluate (poses-<id>.txt, cloud-<id>.ply)")
    ap.add_argument("--ref", help="export directory of the reference run")
    ap.add_argument("--gt", help="TUM ground truth of the camera (groundtruth.txt): evaluates the background trajectory of --est")
    ap.add_argument("--radius", type=float, default=0.05, help="nearest-neighbour search radius in metres (default 0.05)")
    ap.add_argument("--tau", default="0.01,0.02,0.05", help="distance thresholds of the fractions and F-scores (default 0.01,0.02,0.05)")
    ap.add_argument("--pair", action="append", default=[], metavar="EST_ID:REF_ID", help="pair models by id explicitly (repeatable)")
    ap.add_argument("--max-dt", type=float, default=0.02, help="timestamp association window in seconds (default 0.02)")
    ap.add_argument("--rpe-delta", type=float, default=1.0, help="RPE delta (default 1.0)")
    ap.add_argument("--rpe-unit", choices=("s", "f"), default="s", help="RPE delta in seconds or frames (default s)")
    ap.add_argument("--register", action="store_true", help="refine the rigid alignment of every compared cloud pair on the GPU before scoring "
                    "(adds cloud_registered and registration; cloud stays as without the flag)")
    ap.add_argument("--register-radius", metavar="R0,R1,...", help="the registration's radii, coarse to fine (default 4, 2 and 1 times --radius)")
    ap.add_argument("--register-iterations", type=int, default=50, help="iteration cap per radius (default 50)")
    ap.add_argument("--point-to-point", action="store_true", help="register point-to-point (for a reference cloud without normals)")
    ap.add_argument("--register-global", nargs="?", const=True, type=float, metavar="VOXEL", help="register without a start: a coarse pose from FPFH "
                    "descriptors of one key point per VOXEL (default --radius) matched on the GPU and a seeded RANSAC, then --register from it "
                    "(implies --register; adds registration.coarse; radii from 1.5 VOXEL down to VOXEL / 2 unless --register-radius is given)")
    ap.add_argument("--register-seed", type=int, default=0, help="seed of --register-global's RANSAC (default 0)")
    ap.add_argument("--ref-cloud", metavar="FILE", help="a single reference PLY (a ground-truth model) for the background cloud of --est")
    ap.add_argument("--init", metavar="FILE", help="with --ref-cloud: text file with the 4 x 4 est -> ref start")
    ap.add_argument("--ref-mesh", metavar="FILE", help="a reference triangle mesh (.ply or .obj) in place of --ref-cloud: accuracy is the exact "
                    "distance to its triangles; its area-uniform samples and face normals serve as the reference cloud everywhere else")
    ap.add_argument("--mesh-density", type=float, metavar="D", help="samples per square metre of --ref-mesh (default 10000)")
    ap.add_argument("--mesh-cell", type=float, metavar="C", help="cell edge of the triangle search structure (default --radius / 2)")
    ap.add_argument("--estimate-normals", nargs="?", const=True, type=float, metavar="R", help="estimate the normals of a reference cloud whose PLY "
                    "has none, on the GPU from neighbourhoods of radius R (default 2 x --radius): --register then runs point-to-plane against it")
    ap.add_argument("--normals", action="store_true", help="add normal_consistency to every cloud comparison in which both clouds have normals "
                    "(read or estimated), under the registered transform when there is one")
    ap.add_argument("--seg-gt", metavar="DIR", help="ground-truth mask images (Mask####.png / .pgm, instance id per pixel) of the sequence: scores "
                    "the Segmentation<tick>.png label images of --est (the -es export)")
    ap.add_argument("--seg-gt-prefix", default="Mask", help="file name prefix of the masks (default Mask)")
    ap.add_argument("--seg-index-width", type=int, default=4, help="digits of the masks' file index (default 4)")
    ap.add_argument("--seg-radius", type=int, help="pixel radius of the boundary measure, 0..16 (default: 0.008 of the image diagonal)")
    ap.add_argument("--seg-void", type=int, help="ground-truth value that marks pixels to leave out (default: none)")
    ap.add_argument("--observed-from", metavar="SEQ", help="the sequence the run saw (a directory or a .klg): adds cloud_observed -- completeness and "
                    "F-score over the reference points the sensor observed (inside a frustum and not behind the measured depth) -- and observed, "
                    "to the background pair 0:0; cloud stays as without the flag.  Only the depth is read, in chunks of frames")
    ap.add_argument("--observed-poses", metavar="FILE", help="TUM file, camera -> reference frame (default: poses-0.txt of --est, carried into the "
                    "reference frame by the est -> ref transform in force: --init or identity, and the registered one for cloud_registered_observed)")
    ap.add_argument("--observed-cal", metavar="FILE", help="calibration file 'fx fy cx cy [w h]' of the sequence (default 528 528 320 240)")
    ap.add_argument("--observed-tol", metavar="A[,R]", help="a point is on the measured surface within A + R * depth metres (default A = --radius, "
                    "R = 0: a reference point farther than the radius behind the surface could not have been paired anyway)")
    ap.add_argument("--observed-rule", choices=("seen", "surface"), help="seen (default): the sensor's ray reached the point's depth in at least K "
                    "frames, on the surface or through it; surface: the point was on the measured surface in at least K frames")
    ap.add_argument("--observed-min-frames", type=int, metavar="K", help="K of --observed-rule (default 1)")
    ap.add_argument("--observed-stride", type=int, metavar="S", help="use every S-th frame (default 1)")
    ap.add_argument("--observed-max-depth", type=float, metavar="D", help="depth beyond D metres is a hole and the frusta end at D (default: no "
                    "limit); with the run's -d, only what the run was allowed to fuse counts as observed")
    ap.add_argument("--observed-time-scale", type=float, metavar="S", help="a frame's timestamp in the sequence times S is the pose file's seconds "
                    "(default 1e-6, what mf_export_poses writes)")
    a = ap.parse_args(argv)
    obs = None
    given = [k for k in ("poses", "cal", "tol", "rule", "min_frames", "stride", "max_depth", "time_scale") if getattr(a, "observed_" + k) is not None]
    if a.observed_from:
        if not (a.ref or a.ref_cloud or a.ref_mesh):
            ap.error("--observed-from needs --ref or --ref-cloud")
        try:
            tol = [float(x) for x in (a.observed_tol or str(a.radius)).split(",")]
        except ValueError:
            ap.error("--observed-tol takes A or A,R")
        if len(tol) not in (1, 2) or not all(math.isfinite(t) and t >= 0 for t in tol):
            ap.error("--observed-tol takes A or A,R, both finite and not negative")
        obs = {"tol_abs": tol[0], "tol_rel": tol[1] if len(tol) == 2 else 0.0, "rule": a.observed_rule or "seen",
               "min_frames": 1 if a.observed_min_frames is None else a.observed_min_frames, "stride": 1 if a.observed_stride is None else a.observed_stride,
               "max_depth": a.observed_max_depth, "time_scale": 1e-6 if a.observed_time_scale is None else a.observed_time_scale}
        if obs["min_frames"] < 1 or obs["stride"] < 1:
            ap.error("--observed-min-frames and --observed-stride take at least 1")
        if obs["max_depth"] is not None and not (math.isfinite(obs["max_depth"]) and obs["max_depth"] > OBSERVED_NEAR):
            ap.error(f"--observed-max-depth takes a finite depth above {OBSERVED_NEAR} m")
        if not (math.isfinite(obs["time_scale"]) and obs["time_scale"] > 0):
            ap.error("--observed-time-scale takes a positive factor")
    elif given:
        ap.error("--observed-" + given[0].replace("_", "-") + " needs --observed-from")
    if a.register_seed != 0 and a.register_global is None:
        ap.error("--register-seed needs --register-global")
    if not a.seg_gt and (a.seg_radius is not None or a.seg_void is not None):
        ap.error("--seg-radius and --seg-void need --seg-gt")
    if a.seg_radius is not None and not 0 <= a.seg_radius <= MAX_RADIUS:
        ap.error(f"--seg-radius takes 0..{MAX_RADIUS}")
    if a.init and not (a.ref_cloud or a.ref_mesh):
        ap.error("--init needs --ref-cloud")
    if a.ref_cloud and a.ref:
        ap.error("give --ref or --ref-cloud, not both")
    if a.ref_mesh and (a.ref or a.ref_cloud):
        ap.error("--ref-mesh takes the place of --ref and --ref-cloud: give one of the three")
    if not a.ref_mesh and (a.mesh_density is not None or a.mesh_cell is not None):
        ap.error("--mesh-density and --mesh-cell need --ref-mesh")
    mesh_density = 10000.0 if a.mesh_density is None else a.mesh_density
    mesh_cell = a.radius / 2 if a.mesh_cell is None else a.mesh_cell
    if a.ref_mesh and not (math.isfinite(mesh_density) and mesh_density > 0 and math.isfinite(mesh_cell) and mesh_cell > 0):
        ap.error("--mesh-density and --mesh-cell take positive numbers")
    global_voxel = None
    if a.register_global is not None:
        global_voxel = a.radius if a.register_global is True else a.register_global
        if not (math.isfinite(global_voxel) and global_voxel > 0):
            ap.error("--register-global takes a positive voxel size")
        if a.init:
            ap.error("--register-global finds the start itself: give it or --init, not both")
        a.register = True
    if not a.register and (a.register_radius or a.point_to_point):
        ap.error("--register-radius and --point-to-point need --register")
    if a.register and not (a.ref or a.ref_cloud or a.ref_mesh):
        ap.error("--register and --register-global need --ref or --ref-cloud")
    if (a.estimate_normals is not None or a.normals) and not (a.ref or a.ref_cloud or a.ref_mesh):
        ap.error("--estimate-normals and --normals need --ref or --ref-cloud")
    normals_radius = None
    if a.estimate_normals is not None:
        normals_radius = 2 * a.radius if a.estimate_normals is True else a.estimate_normals
        if not (math.isfinite(normals_radius) and normals_radius > 0):
            ap.error("--estimate-normals takes a positive radius")
    taus = tuple(float(x) for x in a.tau.split(",") if x.strip())
    if a.register:
        try:
            radii = [float(x) for x in a.register_radius.split(",") if x.strip()] if a.register_radius else [4 * a.radius, 2 * a.radius, a.radius]
        except ValueError:
            ap.error("--register-radius takes comma-separated numbers")
        if not radii or not all(math.isfinite(r) and r > 0 for r in radii) or a.register_iterations < 1:
            ap.error("--register-radius needs positive radii, --register-iterations at least 1")

    tm = [None]      # --ref-mesh: the TriMesh every cloud* block is scored against

    def compare(ce, cr, T=None, ref_keep=None):
        if tm[0] is not None:
            return compare_cloud_mesh(ce, tm[0], cr, a.radius, taus, T=T, ref_keep=ref_keep)
        return compare_clouds(ce, cr, a.radius, taus, T=T, ref_keep=ref_keep)

    def ref_normals(o, cr, nr):
        """the reference's normals: the file's, or with --estimate-normals and none in the file the estimated ones (recorded in o)"""
        if nr is None and normals_radius is not None and (a.normals or (a.register and not a.point_to_point)):
            nr = estimate_normals(cr, normals_radius)[0]
            o["reference_normals"] = {"estimated": True, "radius": normals_radius, "without_normal": int(np.count_nonzero(np.isnan(nr).any(1)))}
        return nr

    def consistency(o, ce, ne, cr, nr, T):
        if a.normals and ne is not None and nr is not None:
            o["normal_consistency"] = normal_consistency(ce, ne, cr, nr, a.radius, T)

    def registered(o, ce, ne, cr, nr, T0):
        """adds registration and cloud_registered to o; False (after a message) when the reference has no normals and point-to-plane is asked"""
        if nr is None and not a.point_to_point:
            sys.stderr.write(f"eval: the reference cloud of model {o['model']} has no normals (nx ny nz): point-to-plane registration needs "
                             "them; give --point-to-point to register without\n")
            return False
        if global_voxel is not None:
            res = register_global(ce, cr, global_voxel, est_normals=ne, ref_normals=nr, seed=a.register_seed, max_iterations=a.register_iterations,
                                  method="point" if a.point_to_point else "plane", schedule=radii if a.register_radius else None)
        else:
            res = register(ce, cr, radii[-1], T0=T0, ref_normals=None if a.point_to_point else nr, max_iterations=a.register_iterations,
                           schedule=radii, method="point" if a.point_to_point else "plane")
        o["cloud_registered"] = compare(ce, cr, T=res["T"])
        o["registration"] = registration_summary(res)
        if global_voxel is not None:
            o["registration"]["coarse"] = coarse_summary(res["coarse"])
        consistency(o, ce, ne, cr, nr, res["T"])
        return observed_part(o, ce, cr, res["T"], "_registered")

    def observed_part(o, ce, cr, T, suffix=""):
        """With --observed-from and for the background pair 0:0 (object models move: they are not culled), adds cloud<suffix>_observed to o: cr
        culled to what the sequence observed, est -> ref being T (None: identity).  The visibility is computed once when the poses are given in
        the reference frame, and once per transform when they are the estimate's.  False (after a message) when it cannot be computed."""
        if obs is None or o["model"] != 0 or o.get("ref_model", 0) != 0:
            return True
        if obs.get("keep") is None or (obs["own_poses"] and suffix):
            try:
                counts, _, info = observe_sequence(cr, a.observed_from, obs["pose_log"], obs["cal"], pose_to_cloud=T if obs["own_poses"] else None,
                                                   tol_abs=obs["tol_abs"], tol_rel=obs["tol_rel"], max_depth=obs["max_depth"], stride=obs["stride"],
                                                   time_scale=obs["time_scale"], max_dt=a.max_dt)
            except (OSError, ValueError, EOFError) as e:
                sys.stderr.write(f"eval: --observed-from: {e}\n")
                return False
            obs["keep"] = observed(counts, obs["rule"], obs["min_frames"])
            summary = dict(visibility_summary(counts, obs["keep"], info["frames_used"]), frames_skipped=info["frames_skipped"], rule=obs["rule"],
                           min_frames=obs["min_frames"], tol_abs=obs["tol_abs"], tol_rel=obs["tol_rel"], max_depth=obs["max_depth"],
                           poses=a.observed_poses or "estimate")
            o["observed" + suffix] = summary
        o["cloud" + suffix + "_observed"] = compare(ce, cr, T=T, ref_keep=obs["keep"])
        return True

    est = _run_files(a.est)
    results = []
    if obs is not None:
        from .io.readers import load_calibration
        obs["own_poses"] = a.observed_poses is None
        if obs["own_poses"] and (0 not in est or "poses" not in est[0]):
            sys.stderr.write(f"eval: --observed-from: {a.est} holds no poses-0.txt; give --observed-poses\n")
            return 2
        try:
            obs["pose_log"] = read_tum(a.observed_poses or est[0]["poses"])
            obs["cal"] = load_calibration(a.observed_cal) if a.observed_cal else (528.0, 528.0, 320.0, 240.0)
        except (OSError, ValueError) as e:
            sys.stderr.write(f"eval: --observed-poses / --observed-cal: {e}\n")
            return 2
    if a.gt:
        gt = read_tum(a.gt)
        if 0 not in est or "poses" not in est[0]:
            sys.stderr.write(f"eval: {a.est} holds no poses-0.txt (background trajectory)\n")
            return 2
        e0 = read_tum(est[0]["poses"])
        gt_res = {"ate": ate(e0, gt, a.max_dt), "rpe": rpe(e0, gt, a.rpe_delta, a.rpe_unit)}
    if a.ref:
        ref = _run_files(a.ref)
        if a.pair:
            pairs = [tuple(int(x) for x in p.split(":")) for p in a.pair]
        else:
            pairs = [(k, k) for k in sorted(set(est) & set(ref))]
        pe, pr = {p[0] for p in pairs}, {p[1] for p in pairs}
        un_e, un_r = sorted(set(est) - pe), sorted(set(ref) - pr)
        if un_e or un_r:
            sys.stderr.write(f"eval: unmatched ids: est {un_e}, ref {un_r}\n")
        for ei, ri in pairs:
            E, R = est.get(ei, {}), ref.get(ri, {})
            o = {"model": ei, "ref_model": ri}
            el = read_tum(E["poses"]) if "poses" in E else None
            rl = read_tum(R["poses"]) if "poses" in R else None
            if el is not None and rl is not None:
                o["trajectory_vs_ref"] = {"ate": ate(el, rl, a.max_dt), "rpe": rpe(el, rl, a.rpe_delta, a.rpe_unit)}
            if "cloud" in E and "cloud" in R:
                (ce, ne), (cr, nr) = read_ply(E["cloud"], normals=True), read_ply(R["cloud"], normals=True)
                if ei != 0 or ri != 0:   # object models: model frame -> world with each run's own obj -> world pose
                    w = _object_to_world(el, rl, a.max_dt) if el is not None and rl is not None else None
                    if w is None:
                        o["cloud_error"] = "no common timestamp in the two pose logs: the object clouds cannot be placed in the world"
                    else:
                        ce, cr = _apply(w[0], ce), _apply(w[1], cr)
                        if nr is not None:
                            nr = (nr.astype(np.float64) @ w[1][:3, :3].T).astype(np.float32)
                        if ne is not None:
                            ne = (ne.astype(np.float64) @ w[0][:3, :3].T).astype(np.float32)
                        o["cloud_pose_time"] = w[2]
                if "cloud_error" not in o:
                    o["cloud"] = compare_clouds(ce, cr, a.radius, taus)
                    if not observed_part(o, ce, cr, None):
                        return 2
                    nr = ref_normals(o, cr, nr)
                    if a.register:
                        if not registered(o, ce, ne, cr, nr, None):
                            return 2
                    else:
                        consistency(o, ce, ne, cr, nr, None)
            if ei == 0 and a.gt:
                o["trajectory_vs_gt"] = gt_res
            results.append(o)
    elif a.ref_cloud or a.ref_mesh:
        if 0 not in est or "cloud" not in est[0]:
            sys.stderr.write(f"eval: {a.est} holds no cloud-0.ply (background map)\n")
            return 2
        try:
            T0 = read_transform(a.init) if a.init else None
        except (OSError, ValueError) as e:
            sys.stderr.write(f"eval: --init: {e}\n")
            return 2
        ce, ne = read_ply(est[0]["cloud"], normals=True)
        if a.ref_mesh:
            from .mesh import read_triangle_mesh
            try:
                rm = read_triangle_mesh(a.ref_mesh)
            except (OSError, ValueError) as e:
                sys.stderr.write(f"eval: --ref-mesh: {e}\n")
                return 2
            tm[0] = TriMesh(rm["vertices"], rm["triangles"], mesh_cell)
            cr, nr, _ = tm[0].sample(mesh_density)
            o = {"model": 0, "ref_mesh": a.ref_mesh}
        else:
            cr, nr = read_ply(a.ref_cloud, normals=True)
            o = {"model": 0, "ref_cloud": a.ref_cloud}
        o["cloud"] = compare(ce, cr, T=T0)
        if not observed_part(o, ce, cr, T0):
            return 2
        nr = ref_normals(o, cr, nr)
        if a.register:
            if not registered(o, ce, ne, cr, nr, T0):
                return 2
        else:
            consistency(o, ce, ne, cr, nr, T0)
        if a.gt:
            o["trajectory_vs_gt"] = gt_res
        results.append(o)
    elif a.gt:
        results.append({"model": 0, "trajectory_vs_gt": gt_res})
    elif not a.seg_gt:
        ap.error("give --ref, --ref-cloud, --ref-mesh, --gt, --seg-gt or a combination")
    if a.seg_gt:
        try:
            results += score_segmentation(a.est, a.seg_gt, a.seg_gt_prefix, a.seg_index_width, a.seg_radius, a.seg_void)
        except (OSError, ValueError) as e:
            sys.stderr.write(f"eval: --seg-gt: {e}\n")
            return 2
    for o in results:
        print(json.dumps(_clean(o)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
