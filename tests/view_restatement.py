"""The definition behind the view scores (include/maskfusion_amd.h: mf_view_score_dev), restated in numpy with the same operation order:
what the tests compare the device kernel with.  Nothing here is shared with the product's code.

Inputs as for the device call: render_rgba uint8 (n_frames, H, W, 4), render_depth float32 (n_frames, H, W), rgb uint8 (n_frames, H, W, 3),
depth float32 (n_frames, H, W), group uint8 (n_frames, H, W) or None.  Every fp64 operation below is one numpy operation on float64
arrays, so each is rounded on its own, as on the device."""
import math

import numpy as np

FIX = float(1 << 24)
C1, C2 = 6.5025, 58.5225
HALO, TAPS = 5, 11


def weights():
    """g[k] = exp(-(k - 5)^2 / 4.5), w[k] = g[k] / (g[0] + ... + g[10]) summed left to right (math.exp: the C library's exp, which the
    host side of the call uses)"""
    g = [math.exp(-float((k - HALO) * (k - HALO)) / 4.5) for k in range(TAPS)]
    total = 0.0
    for v in g:
        total = total + v
    return [v / total for v in g]


def filtered(q, w):
    """q (H, W) float64 filtered along the row, then the row results along the column: (H - 10, W - 10), one value per pixel whose window
    lies inside the image.  acc = 0; for k = 0..10: acc = acc + w[k] * q[col - 5 + k]"""
    H, W = q.shape
    row = np.zeros((H, W - 2 * HALO))
    for k in range(TAPS):
        row = row + w[k] * q[:, k:k + W - 2 * HALO]
    out = np.zeros((H - 2 * HALO, W - 2 * HALO))
    for k in range(TAPS):
        out = out + w[k] * row[k:k + H - 2 * HALO, :]
    return out


def ssim_channel(xb, yb, w):
    """SSIM of one channel, bytes xb (render) against yb (input), at every pixel whose 11 x 11 window lies inside the image"""
    x, y = xb.astype(np.float64), yb.astype(np.float64)
    mx, my, exx, exy, eyy = filtered(x, w), filtered(y, w), filtered(x * x, w), filtered(x * y, w), filtered(y * y, w)
    vx = exx - mx * mx
    vy = eyy - my * my
    cxy = exy - mx * my
    num = (2.0 * mx * my + C1) * (2.0 * cxy + C2)
    den = (mx * mx + my * my + C1) * (vx + vy + C2)
    return num / den


def ssim_fixed(render_rgb, rgb):
    """int64 (H, W): llrint(s 2^24) with s = (s_R + s_G + s_B) / 3.0 where the window lies inside the image, 0 elsewhere; and that mask"""
    H, W = rgb.shape[:2]
    fixed, inside = np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    if H >= TAPS and W >= TAPS:
        w = weights()
        s = [ssim_channel(render_rgb[:, :, c], rgb[:, :, c], w) for c in range(3)]
        mean = (s[0] + s[1] + s[2]) / 3.0
        fixed[HALO:H - HALO, HALO:W - HALO] = np.rint(mean * FIX).astype(np.int64)      # (rint: to nearest, ties to even, like llrint)
        inside[HALO:H - HALO, HALO:W - HALO] = True
    return fixed, inside


def counts(render_rgba, render_depth, rgb, depth, group=None, n_groups=1, max_depth=np.inf, tau=0.01):
    """uint64 [n_frames][n_groups][10], counter 9 a two's-complement int64"""
    render_rgba, rgb = np.asarray(render_rgba, np.uint8), np.asarray(rgb, np.uint8)
    render_depth, depth = np.asarray(render_depth, np.float32), np.asarray(depth, np.float32)
    F, H, W = depth.shape
    tau32, max32 = np.float32(tau), np.float32(min(float(max_depth), float(np.finfo(np.float32).max)))
    out = np.zeros((F, n_groups, 10), np.int64)
    for f in range(F):
        g = np.zeros((H, W), np.int64) if group is None else np.asarray(group[f]).astype(np.int64)
        zr, zi = render_depth[f], depth[f]
        with np.errstate(invalid="ignore"):
            covered = np.isfinite(zr) & (zr > 0)
            valid = np.isfinite(zi) & (zi > 0) & (zi <= max32)
            pair = covered & valid
            dz = np.abs(np.where(pair, zr, np.float32(0)) - np.where(pair, zi, np.float32(0)))      # one fp32 subtraction
        assert dz.dtype == np.float32
        within = pair & (dz <= tau32)
        l1 = np.where(pair, np.rint(dz.astype(np.float64) * FIX), 0.0).astype(np.int64)
        d = render_rgba[f][:, :, :3].astype(np.int64) - rgb[f].astype(np.int64)
        sq = (d * d).sum(2)
        fixed, inside = ssim_fixed(render_rgba[f][:, :, :3], rgb[f])
        for k in range(n_groups):
            m = g == k
            out[f, k] = [m.sum(), (m & covered).sum(), (m & valid).sum(), (m & pair).sum(), (m & within).sum(), l1[m].sum(), sq[m].sum(),
                         sq[m & covered].sum(), (m & inside).sum(), fixed[m & inside].sum()]
    return out.view(np.uint64)
