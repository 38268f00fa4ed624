"""Recognition of a returning object: is the map of a NEW object model the map of an archived, inactive one (MaskFusion::redetectModels /
Model::detectInRegion upstream, which the release ships empty)?  Two downloadMap arrays are registered without a start --
maskfusion_amd.eval.register_global with the hypothesis search on the GPU (mf_pose_ransac_dev) and a point-to-plane finish -- and the result
is accepted by two thresholds.  DESIGN.md "Inactive models and re-detection" has the measurements behind the defaults."""
from __future__ import annotations

import numpy as np

from . import eval as ev

VOXEL_FRACTION = 1.0 / 40.0        # voxel = this share of the archived cloud's bounding-box diagonal
MIN_SHARE = 0.91                   # of the new map's points, within voxel / 2 of the archived map under the final pose


def _cloud(records):
    r = np.asarray(records, np.float32).reshape(-1, 12)
    return np.ascontiguousarray(r[:, :3]), np.ascontiguousarray(r[:, 8:11])


def default_voxel(old_records, fraction: float = VOXEL_FRACTION) -> float:
    p = _cloud(old_records)[0]
    p = p[np.isfinite(p).all(1)]
    if len(p) == 0:
        return 0.0
    return float(fraction * np.linalg.norm(p.max(0).astype(np.float64) - p.min(0).astype(np.float64)))


def match_model(new_records, old_records, voxel=None, seed: int = 0, hypotheses: int = 20000, min_share: float = MIN_SHARE,
                fraction: float = VOXEL_FRACTION) -> dict:
    """new_records, old_records: (n, 12) float32 as Model.downloadMap returns them; positions (columns 0..2) and normals (8..10) are used,
    both in their model's own coordinates.  voxel: the key-point spacing of register_global, by default `fraction` of the archived cloud's
    bounding-box diagonal.  Returns {"T": 4 x 4 fp64, new -> old (old = T new), "inlier_share": the share of the new map's points with a
    partner in the old map within voxel / 2 under T, "rmse": of those pairs (None without any), "accepted": inlier_share >= min_share and
    rmse <= voxel / 2, "voxel", "converged", "reason", "coarse"}.  Too few points on either side: not accepted, T the identity."""
    pn, nn = _cloud(new_records)
    po, no = _cloud(old_records)
    voxel = default_voxel(old_records, fraction) if voxel is None else float(voxel)
    out = {"T": np.eye(4), "inlier_share": 0.0, "rmse": None, "accepted": False, "voxel": voxel, "converged": False, "reason": "too few points",
           "coarse": None}
    if len(pn) < 3 or len(po) < 3 or not voxel > 0:
        return out
    res = ev.register_global(pn, po, voxel, est_normals=nn, ref_normals=no, seed=seed, hypotheses=hypotheses, ransac="device", method="plane")
    share, rmse = float(res["inlier_share"]), res["rmse"]
    out.update({"T": np.asarray(res["T"], np.float64), "inlier_share": share, "rmse": None if rmse is None else float(rmse),
                "converged": bool(res["converged"]), "reason": res["reason"], "coarse": res["coarse"]})
    out["accepted"] = bool(rmse is not None and share >= min_share and float(rmse) <= voxel / 2.0)
    return out
