"""The definition behind the cloud visibility (include/maskfusion_amd.h: mf_cloud_visibility_dev), restated in numpy float32 with the same
operation order: what the tests compare the device kernel with.  Nothing here is shared with the product's code and nothing calls the library.

points (n, >= 3) float32, x y z first; depth float32 (n_frames, H, W) in metres; cam_from_cloud float32 (n_frames, 12), the rows of each frame's
3 x 4.  Every fp32 operation below is one numpy operation on float32 arrays, so each is rounded on its own, as on the device; the loop runs
over the frames."""
import numpy as np

IN_FRUSTUM, ON_SURFACE, SEEN_THROUGH, OCCLUDED = 0, 1, 2, 3
NONE, HOLE = -1, -2          # classify(): not in the frustum; in the frustum with a sample that is not valid


def classify(points, depth_frame, M, fx, fy, cx, cy, near_z, far_z, tol_abs, tol_rel):
    """int8 (n,) for ONE frame: NONE, HOLE, ON_SURFACE, SEEN_THROUGH or OCCLUDED"""
    f32 = np.float32
    p = np.asarray(points, f32)
    d_img = np.asarray(depth_frame, f32)
    H, W = d_img.shape
    M = np.asarray(M, f32).reshape(12)
    fx, fy, cx, cy, near_z, far_z, tol_abs, tol_rel = (f32(v) for v in (fx, fy, cx, cy, near_z, far_z, tol_abs, tol_rel))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.full(len(p), NONE, np.int8)
    with np.errstate(all="ignore"):
        xc = ((M[0] * x + M[1] * y) + M[2] * z) + M[3]
        yc = ((M[4] * x + M[5] * y) + M[6] * z) + M[7]
        zc = ((M[8] * x + M[9] * y) + M[10] * z) + M[11]
        front = (zc > near_z) & (zc <= far_z)
        u = fx * (xc / zc) + cx
        v = fy * (yc / zc) + cy
        col = np.floor(u + f32(0.5))
        row = np.floor(v + f32(0.5))
        assert xc.dtype == zc.dtype == u.dtype == col.dtype == np.float32
        inside = front & (col >= f32(0)) & (col < f32(W)) & (row >= f32(0)) & (row < f32(H))       # as floats: NaN and +-inf fail
        idx = np.flatnonzero(inside)
        d = d_img[row[idx].astype(np.int64), col[idx].astype(np.int64)]
        valid = np.isfinite(d) & (d > f32(0))
        tol = tol_abs + tol_rel * d
        dz = zc[idx] - d
        assert tol.dtype == dz.dtype == np.float32
        cls = np.full(len(idx), HOLE, np.int8)
        cls[valid & (np.abs(dz) <= tol)] = ON_SURFACE
        cls[valid & (dz < -tol)] = SEEN_THROUGH
        cls[valid & (dz > tol)] = OCCLUDED
    out[idx] = cls
    return out


def visibility(points, depth, cam_from_cloud, fx, fy, cx, cy, near_z, far_z, tol_abs, tol_rel, frame_base=0, counts=None, first=None):
    """(counts uint32 (n, 4) = {in frustum, on surface, seen through, occluded}, first int32 (n,) = the smallest frame_base + f with ON SURFACE
    or -1).  With counts and first given, the call accumulates onto copies of them: the counts are added, a first >= 0 is kept."""
    n = len(points)
    depth = np.asarray(depth, np.float32)
    cam = np.asarray(cam_from_cloud, np.float32).reshape(len(depth), 12)
    counts = np.zeros((n, 4), np.uint32) if counts is None else np.array(counts, np.uint32)
    first = np.full(n, -1, np.int32) if first is None else np.array(first, np.int32)
    for f in range(len(depth)):
        c = classify(points, depth[f], cam[f], fx, fy, cx, cy, near_z, far_z, tol_abs, tol_rel)
        counts[:, IN_FRUSTUM] += (c != NONE)
        for k in (ON_SURFACE, SEEN_THROUGH, OCCLUDED):
            counts[:, k] += (c == k)
        first[(c == ON_SURFACE) & (first < 0)] = frame_base + f
    return counts, first


def categories(counts):
    """how many points were: never in a frustum; in one but only ever in holes; on surface at least once; seen through at least once;
    occluded at least once"""
    c = np.asarray(counts).astype(np.int64)
    return {"never": int(np.count_nonzero(c[:, 0] == 0)), "hole": int(np.count_nonzero((c[:, 0] > 0) & (c[:, 1:].sum(1) == 0))),
            "on": int(np.count_nonzero(c[:, 1])), "through": int(np.count_nonzero(c[:, 2])), "occluded": int(np.count_nonzero(c[:, 3]))}
