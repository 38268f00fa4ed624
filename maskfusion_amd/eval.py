"""Run evaluation: trajectories (TUM-style ATE / RPE) and maps (accuracy / completeness / F-score by GPU nearest-surfel distances).

Reads what a run writes -- poses-<id>.txt (mf_export_poses; TUM `ts tx ty tz qx qy qz qw`, also a TUM groundtruth.txt) and cloud-<id>.ply
(mf_save_ply; binary little endian, or ASCII PLY with x / y / z) -- from this library or from the reference.  The cloud distances run on the
GPU through mf_cloud_nn_dev (kernels: csrc/mf_eval.hip); everything else is numpy.

    python -m maskfusion_amd.eval --est DIR [--ref DIR] [--gt FILE] [--radius R] [--tau a,b,c] [--pair est_id:ref_id ...]

prints one JSON object per model on stdout (INTEGRATION.md "Evaluating a run").
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


def read_ply(path: str) -> np.ndarray:
    """The vertex positions of a PLY file, (n, 3) float32: binary little endian (mf_save_ply's and the reference's layout) or ASCII.
    The vertex element must come first; other elements after it are ignored."""
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
    if fmt == "binary_little_endian":
        dt = np.dtype([(nm, "<" + t) for nm, t in props])
        v = np.frombuffer(raw, dt, count=n, offset=body_at)
        return np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)
    if fmt == "ascii":
        lines = raw[body_at:].decode("ascii").split("\n")
        rows = [l.split() for l in lines if l.strip()][:n]
        a = np.array(rows, np.float64).reshape(n, len(props))
        return a[:, [names.index("x"), names.index("y"), names.index("z")]].astype(np.float32)
    raise ValueError(f"{path}: format {fmt} is not supported")


def _device_points(a):
    """(tensor on the library's device, stride in floats)"""
    import torch
    from .lib import torch_device
    if isinstance(a, torch.Tensor):
        t = a
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32)))
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < 3:
        raise ValueError("points must be (n, >= 3) float32")
    return t.to(torch_device()).contiguous()


def nearest(target, query, radius: float, T=None):
    """For every query point the nearest target point within `radius` (mf_cloud_nn_dev on device buffers).  target, query: (n, >= 3)
    float32 numpy arrays or device tensors (x, y, z first); T: 4 x 4 applied to the queries first.  Returns numpy (dist float32, +inf: none
    in range; idx int32, -1: none)."""
    import torch
    from .lib import load, MFError
    L = load()
    t, q = _device_points(target), _device_points(query)
    nt, nq = int(t.shape[0]), int(q.shape[0])
    need = C.c_uint64(0)
    if L.mf_cloud_nn_workspace(nt, C.byref(need)) != 0:
        raise MFError("mf_cloud_nn_workspace failed")
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=q.device)
    dist = torch.empty(max(nq, 1), dtype=torch.float32, device=q.device)
    idx = torch.empty(max(nq, 1), dtype=torch.int32, device=q.device)
    T16 = None if T is None else np.ascontiguousarray(np.asarray(T, np.float32).T.reshape(16))
    stream = torch.cuda.current_stream().cuda_stream if q.device.type == "cuda" else None
    rc = L.mf_cloud_nn_dev(t.data_ptr() if nt else None, int(t.shape[1]), nt, q.data_ptr() if nq else None, int(q.shape[1]), nq,
                           T16.ctypes.data if T16 is not None else None, float(radius), dist.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                           int(need.value), stream)
    if rc != 0:
        raise MFError(f"mf_cloud_nn_dev failed with code {rc} (radius must be finite and > 0, coordinates |x / radius| < 2^30)")
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


def compare_clouds(est, ref, radius: float = 0.05, taus=(0.01, 0.02, 0.05)) -> dict:
    """accuracy = est -> ref distances, completeness = ref -> est, and F-score(tau) = 2 P R / (P + R) with P, R their fractions <= tau"""
    acc = cloud_stats(nearest(ref, est, radius)[0], radius, taus)
    comp = cloud_stats(nearest(est, ref, radius)[0], radius, taus)
    f = {}
    for t in taus:
        k = f"{t:g}"
        p, r = acc["fraction"][k], comp["fraction"][k]
        f[k] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return {"radius": radius, "accuracy": acc, "completeness": comp, "fscore": f}


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
    a = ap.parse_args(argv)
    taus = tuple(float(x) for x in a.tau.split(",") if x.strip())
    est = _run_files(a.est)
    results = []
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
                ce, cr = read_ply(E["cloud"]), read_ply(R["cloud"])
                if ei != 0 or ri != 0:   # object models: model frame -> world with each run's own obj -> world pose
                    w = _object_to_world(el, rl, a.max_dt) if el is not None and rl is not None else None
                    if w is None:
                        o["cloud_error"] = "no common timestamp in the two pose logs: the object clouds cannot be placed in the world"
                    else:
                        ce, cr = _apply(w[0], ce), _apply(w[1], cr)
                        o["cloud_pose_time"] = w[2]
                if "cloud_error" not in o:
                    o["cloud"] = compare_clouds(ce, cr, a.radius, taus)
            if ei == 0 and a.gt:
                o["trajectory_vs_gt"] = gt_res
            results.append(o)
    elif a.gt:
        results.append({"model": 0, "trajectory_vs_gt": gt_res})
    else:
        ap.error("give --ref, --gt or both")
    for o in results:
        print(json.dumps(_clean(o)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
