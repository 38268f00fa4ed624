"""The two definitions behind the segmentation scores (include/maskfusion_amd.h: mf_label_confusion_dev, mf_label_boundary_dev), restated in
numpy by brute force: what the tests compare the device kernels with.  Nothing here is shared with the product's code.

Inputs as for the device calls: est, gt uint8 (n_frames, H, W); lut_est, lut_gt 256 entries, a raw value -> a class index or 255 (void)."""
import numpy as np

VOID = 255


def confusion(est, gt, lut_est, lut_gt, n_est, n_gt):
    """uint32 [n_frames][n_gt][n_est]: the pixels of frame f whose ground truth maps to g and whose estimate maps to e; a pixel that is
    void on either side is counted nowhere"""
    est, gt = np.asarray(est, np.uint8), np.asarray(gt, np.uint8)
    ce, cg = np.asarray(lut_est, np.uint8)[est].astype(np.int64), np.asarray(lut_gt, np.uint8)[gt].astype(np.int64)
    out = np.zeros((est.shape[0], n_gt, n_est), np.uint32)
    for f in range(est.shape[0]):
        ok = (ce[f] != VOID) & (cg[f] != VOID)
        out[f] = np.bincount(cg[f][ok] * n_est + ce[f][ok], minlength=n_gt * n_est).reshape(n_gt, n_est)
    return out


def boundary_mask(cls, k):
    """Pixel p is a boundary pixel of class k in a label image if its label maps to k and at least one of its 4-neighbours inside the
    image maps to something else, void included.  The image border by itself makes no boundary.  cls: (H, W) compact classes."""
    mine = cls == k
    other = np.zeros_like(mine)
    other[:, 1:] |= cls[:, :-1] != cls[:, 1:]      # the left neighbour differs
    other[:, :-1] |= cls[:, 1:] != cls[:, :-1]     # the right one
    other[1:, :] |= cls[:-1, :] != cls[1:, :]      # the one above
    other[:-1, :] |= cls[1:, :] != cls[:-1, :]     # the one below
    return mine & other


def hits(a, b, radius):
    """how many pixels set in a have a pixel set in b at dx^2 + dy^2 <= radius^2 (integers; radius 0: the same pixel): an explicit loop
    over the disc's offsets"""
    H, W = a.shape
    if not a.any() or not b.any():
        return 0
    near = np.zeros_like(a)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dx * dx + dy * dy > radius * radius:
                continue
            # near[y, x] |= b[y + dy, x + dx] where that lies inside the image
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
            yd, xd = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
            near[ys, xs] |= b[yd, xd]
    return int(np.count_nonzero(a & near))


def boundary(est, gt, lut_est, lut_gt, n_gt, pair, radius):
    """uint32 [n_frames][n_gt][4] = {n_est_boundary, est_hit, n_gt_boundary, gt_hit}; for g with pair[g] = 255: {0, 0, n_gt_boundary, 0}.
    A void pixel is a boundary pixel of nothing (k never equals 255 here)."""
    est, gt = np.asarray(est, np.uint8), np.asarray(gt, np.uint8)
    ce, cg = np.asarray(lut_est, np.uint8)[est], np.asarray(lut_gt, np.uint8)[gt]
    out = np.zeros((est.shape[0], n_gt, 4), np.uint32)
    for f in range(est.shape[0]):
        for g in range(n_gt):
            bg = boundary_mask(cg[f], g)
            out[f, g, 2] = np.count_nonzero(bg)
            e = int(pair[g])
            if e == VOID:
                continue
            be = boundary_mask(ce[f], e)
            out[f, g, 0] = np.count_nonzero(be)
            out[f, g, 1] = hits(be, bg, radius)
            out[f, g, 3] = hits(bg, be, radius)
    return out
