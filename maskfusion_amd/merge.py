"""Map merging: the surfels of one map, moved by a rigid transform, fused into another map on the GPU (mf_cloud_merge_dev, kernels:
csrc/mf_merge.hip; DESIGN.md "Map merging").  merge_maps() works on two downloadMap arrays; Model.mergeMap (maskfusion_amd.api) on a live
model; the command joins the background maps of two saved sessions:

    python -m maskfusion_amd.merge --a A.mfs --b B.mfs (--init T.txt | --register-global VOXEL) [--radius R] [--min-cos C] -o merged.mfs
                                   [--ply merged.ply]

B's background map (model 0) goes into A's, under the transform T from B's world to A's: the 4 x 4 of --init (maskfusion_amd.eval's file
format) or the result of maskfusion_amd.eval.register_global on the two maps, point-to-plane finish included.  A is saved with the merged map
(its user blob unchanged), and one JSON line is printed: the four counts, n_out, the radius and the registration's inlier share and rmse."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

COS_HALF_RAD = np.float32(math.cos(0.5))       # the association's normal gate: angleBetween(...) < 0.5 rad (Core/Shaders/data.vert:153)


def default_radius(target) -> float:
    """twice the median of the target's finite radii (column 11); 0.0 for a map without any.  A definition: nobody has measured it against
    real maps (DESIGN.md "Map merging")"""
    r = np.asarray(target, np.float32).reshape(-1, 12)[:, 11]
    r = r[np.isfinite(r)]
    return float(2.0 * np.median(r.astype(np.float64))) if len(r) else 0.0


def rewrite_stamps(records, tick_a: int, tick_b: int) -> np.ndarray:
    """B's records with initTime and lastTime (columns 6, 7) on A's clock: clip(stamp + (tick_a - tick_b), 1, tick_a).  Stamps <= 0 and stamps
    in the future have meanings of their own in Model::clean, so none is left.  tick_a must be at least 1."""
    if int(tick_a) < 1:
        raise ValueError("the target session has processed no frame: its tick must be at least 1")
    r = np.array(records, np.float32).reshape(-1, 12)
    r[:, 6:8] = np.clip(r[:, 6:8].astype(np.float64) + (int(tick_a) - int(tick_b)), 1, int(tick_a)).astype(np.float32)
    return r


def merge_maps(target, source, T=None, radius=None, min_cos=COS_HALF_RAD):
    """mf_cloud_merge_dev on two (n, 12) float32 maps in Model.downloadMap's layout (numpy arrays, or tensors on the library's device).
    T: 4 x 4, source -> target (None: none); radius: the partner search's (None: default_radius(target)); min_cos: the gate on the two
    normals' dot product.  Returns (records (n_out, 12) float32, stats [averaged, confidence only, appended, dropped], match int32
    (n_source,): the partner's index, -1 appended, -2 dropped), all numpy."""
    import torch
    from . import eval as ev
    from .lib import load
    L = load()
    what = "maps must be (n, 12) float32"
    t, s = ev._device_points(target, 12, what), ev._device_points(source, 12, what)
    if t.shape[1] != 12 or s.shape[1] != 12:
        raise ValueError(what)
    nt, ns = int(t.shape[0]), int(s.shape[0])
    if radius is None:
        radius = default_radius(t.cpu().numpy())
        if not radius > 0:
            raise ValueError("the target map has no finite radius to derive the search radius from: give one")
    ws, need = ev._workspace(L, "mf_cloud_merge_workspace", t.device, nt, ns)
    out = torch.empty((max(nt + ns, 1), 12), dtype=torch.float32, device=t.device)
    match = torch.empty(max(ns, 1), dtype=torch.int32, device=t.device)
    n_out, stats = C.c_int64(0), (C.c_uint64 * 4)()
    T16 = ev._pack_T(T)
    rc = L.mf_cloud_merge_dev(t.data_ptr() if nt else None, nt, s.data_ptr() if ns else None, ns, T16.ctypes.data if T16 is not None else None,
                              float(radius), float(min_cos), out.data_ptr(), nt + ns, C.byref(n_out), match.data_ptr(), stats, ws.data_ptr(), need,
                              ev._stream_of(t.device))
    ev._check(rc, "mf_cloud_merge_dev", "radius must be finite and > 0, min_cos in [-1, 1], a finite transform, coordinates |x / radius| < 2^30")
    return out[:n_out.value].cpu().numpy(), [int(v) for v in stats], match[:ns].cpu().numpy()


def join_maps(map_a, map_b, T, tick_a: int, tick_b: int, radius=None, min_cos=COS_HALF_RAD, merge=merge_maps):
    """what the command does to the two background maps: B's stamps onto A's clock, then `merge` (merge_maps, or a stand-in with its
    signature).  Returns (records, stats, match, radius)"""
    radius = default_radius(map_a) if radius is None else float(radius)
    rec, stats, match = merge(map_a, rewrite_stamps(map_b, tick_a, tick_b), T, radius, min_cos)
    return rec, stats, match, radius


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m maskfusion_amd.merge", description="merge the background map of session B into session A")
    ap.add_argument("--a", required=True, metavar="A.mfs", help="the session that receives the map")
    ap.add_argument("--b", required=True, metavar="B.mfs", help="the session whose background map (model 0) is merged into A's")
    ap.add_argument("--init", metavar="T.txt", help="text file with the 4 x 4 transform from B's world to A's")
    ap.add_argument("--register-global", type=float, metavar="VOXEL", help="find the transform: maskfusion_amd.eval.register_global on the two maps "
                    "with this key-point spacing in metres, point-to-plane finish included")
    ap.add_argument("--radius", type=float, help="partner search radius in metres (default: twice the median radius of A's surfels)")
    ap.add_argument("--min-cos", type=float, default=float(COS_HALF_RAD), help="smallest dot product of two partners' normals (default cos 0.5)")
    ap.add_argument("-o", "--out", required=True, metavar="merged.mfs", help="where A is saved with the merged map")
    ap.add_argument("--ply", metavar="merged.ply", help="also write the merged map as a point cloud")
    return ap


def parse(argv=None):
    """the arguments, checked: everything that can be refused without a GPU is refused here (exit status 2)"""
    ap = parser()
    a = ap.parse_args(argv)
    if (a.init is None) == (a.register_global is None):
        ap.error("give --init or --register-global, one of the two")
    if a.register_global is not None and not (math.isfinite(a.register_global) and a.register_global > 0):
        ap.error("--register-global takes a positive voxel size")
    if a.radius is not None and not (math.isfinite(a.radius) and a.radius > 0):
        ap.error("--radius takes a positive number")
    if not (math.isfinite(a.min_cos) and -1.0 <= a.min_cos <= 1.0):
        ap.error("--min-cos takes a number in [-1, 1]")
    for f in (a.a, a.b) + ((a.init,) if a.init else ()):
        if not os.path.isfile(f):
            ap.error(f"{f}: no such file")
    a.T = None
    if a.init:
        from . import eval as ev
        try:
            a.T = ev.read_transform(a.init)
        except ValueError as e:
            ap.error(str(e))
    return a


def write_cloud(path: str, records):
    """the records as a PLY cloud: positions, colours and, as mf_save_ply writes them, the normals negated"""
    from .mesh import write_mesh_ply
    r = np.asarray(records, np.float32).reshape(-1, 12)
    col = np.nan_to_num(r[:, 4]).astype(np.int64)
    write_mesh_ply(path, r[:, :3], -r[:, 8:11], np.stack([col >> 16 & 0xFF, col >> 8 & 0xFF, col & 0xFF], 1).astype(np.float32))


def main(argv=None) -> int:
    a = parse(argv)
    from . import eval as ev
    from .api import MaskFusion
    from .lib import MFError
    A = B = None
    try:
        A, B = MaskFusion.loadSession(a.a), MaskFusion.loadSession(a.b)
        tick_a, tick_b = A.getTick(), B.getTick()
        map_a, map_b = A.getBackgroundModel().downloadMap(), B.getBackgroundModel().downloadMap()
        B.close()
        B = None
        share = rmse = None
        T = a.T
        if T is None:
            res = ev.register_global(map_b[:, :3], map_a[:, :3], a.register_global, est_normals=map_b[:, 8:11], ref_normals=map_a[:, 8:11], method="plane")
            T, share, rmse = np.asarray(res["T"], np.float64), float(res["inlier_share"]), None if res["rmse"] is None else float(res["rmse"])
        radius = default_radius(map_a) if a.radius is None else a.radius
        stats = A.getBackgroundModel().mergeMap(rewrite_stamps(map_b, tick_a, tick_b), T=T, radius=radius, min_cos=a.min_cos)
        n_out = A.getBackgroundModel().lastCount()
        A.saveSession(a.out, user=MaskFusion.sessionInfo(a.a)["user"])
        if a.ply:
            write_cloud(a.ply, A.getBackgroundModel().downloadMap())
    except (MFError, ValueError, OSError) as e:
        sys.stderr.write(f"merge: {e}\n")
        return 1
    finally:
        for m in (A, B):
            if m is not None:
                m.close()
    print(json.dumps({"averaged": stats[0], "confidence_only": stats[1], "appended": stats[2], "dropped": stats[3], "n_out": n_out,
                      "radius": float(radius), "inlier_share": share, "rmse": rmse}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
