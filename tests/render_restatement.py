"""A from-scratch numpy restatement of the headless render (DESIGN.md "Rendering", include/maskfusion_amd.h mf_render_view): the maps as
Model.downloadMap returns them, the poses, ids, class ids and thresholds read through the API, one virtual pinhole camera.

Every pixel gets the winner's colour, camera z and model list index, and a flag that says whether the pixel is AMBIGUOUS: the best two
candidate depths lie within DEPTH_EPS relative and would draw different things, or a candidate that could win sits within 1e-5 of the disc's rim (+ fp32's cancellation, see below) (or of near / far, or meets the disc at a
grazing angle, or -- points mode -- lies within 1e-4 px of a pixel border).  Such a pixel may go either way under fp32 rounding; the tests compare the others exactly.
"""
from __future__ import annotations

import numpy as np

EPS = 1e-5          # rim, near / far and pixel-border margin
# Depth ties: two candidates closer than this (relative) may swap under fp32.  The device's depths agree with this float64 restatement to
# ~1e-6 relative (the view transform is composed in fp32 there); 1e-5 flagged ~0.4 % of a VGA render of a fused map, whose overlapping
# coplanar discs meet a ray within a few 1e-6 of each other everywhere -- 2e-6 is twice the disagreement measured.
DEPTH_EPS = 2e-6
# fp32 error of a ray-plane depth relative to the depth, per 1 / |cos| of the angle between ray and disc normal (the transforms and the plane
# offset carry ~1e-7 relative each)
GRAZE = 2e-7


def model_transforms(mf, view):
    """list index -> model -> view (4 x 4 float64): the background in world coordinates, an object through bgPose . pose^-1"""
    Vi = np.linalg.inv(view.pose())
    models = mf.getModels()
    bg = models[0].getPose()
    out = []
    for i, m in enumerate(models):
        out.append(Vi if i == 0 else Vi @ bg @ np.linalg.inv(m.getPose()))
    return out


def _colour(ctype, s, tick, is_bg, class_id, palette, points, unstable, draw_window, time_delta):
    n = s[:, 8:11].astype(np.float64)
    ci = s[:, 4].astype(np.int64)
    dec = np.stack([(ci >> 16) & 255, (ci >> 8) & 255, ci & 255], 1).astype(np.float64) / 255.0
    dn = np.abs(n.sum(1))[:, None]
    grey = np.repeat(0.5 * dn + 0.1, 3, 1)
    if points:
        return n if ctype == 1 else dec if ctype == 2 else grey
    c = grey.copy()
    if ctype == 1:
        c = n.copy()
    elif ctype == 2:
        c = dec.copy()
    else:
        ratio = 2.0 * (s[:, 6].astype(np.float64) - 1.0) / (float(tick) - 1.0)
        r0 = np.fmax(0.0, 1.0 - ratio)
        r1 = np.fmax(0.0, ratio - 1.0)
        times = np.stack([r0, r1, 1.0 - r0 - r1], 1) * (dn + 0.1)
        use_t = unstable | (ctype == 3)
        if ctype == 4:
            if is_bg:
                lab = np.repeat(0.5 * dn + 0.5, 3, 1)
            else:
                q = class_id % len(palette)
                lab = np.asarray(palette, np.float64)[q][None, :] * np.fmax(dn, 0.8)
            c = lab
        c = np.where(use_t[:, None], times, c)
    if draw_window:
        c = np.where(((float(tick) - s[:, 7]) > time_delta)[:, None], c * 0.25, c)
    return c


def render(mf, view, palette=None, time_delta=200):
    """-> rgba (H, W, 4) uint8, depth (H, W) float64 (0: none), model (H, W) int32 (-1: none), ambiguous (H, W) bool"""
    W, H = int(view.width), int(view.height)
    fx, fy, cx, cy, near, far = (float(view.fx), float(view.fy), float(view.cx), float(view.cy), float(view.near_z), float(view.far_z))
    points = bool(view.draw_points)
    tick = mf.getTick()
    models = mf.getModels()
    Ms = model_transforms(mf, view)
    cand_p, cand_z, cand_ord, cand_m, cand_q, cand_c, cand_cos = [], [], [], [], [], [], []
    order_base = 0
    for i, m in enumerate(models):
        if not (view.draw_background if i == 0 else view.draw_objects):
            continue
        if view.model_mask and not (int(view.model_mask) >> i) & 1:
            continue
        s = m.downloadMap().astype(np.float64)
        info = m.info()
        thr = float(info.confidence_threshold)
        M = Ms[i]
        conf = s[:, 3] > thr
        keep = conf if points else (conf | bool(view.draw_unstable))
        idx = np.nonzero(keep)[0]
        s = s[idx]
        ctype = view.background_color_type if i == 0 else view.object_color_type
        col = _colour(ctype, s, tick, i == 0, int(info.class_id), palette, points, ~(s[:, 3] > thr), bool(view.draw_window) and not points,
                      time_delta)
        h = s[:, :3] @ M[:3, :3].T + M[:3, 3]
        if points:
            ok = (h[:, 2] >= near) & (h[:, 2] <= far)
            u = fx * h[:, 0] / h[:, 2] + cx
            v = fy * h[:, 1] / h[:, 2] + cy
            ok &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
            k = np.nonzero(ok)[0]
            px, py = np.floor(u[k]).astype(np.int64), np.floor(v[k]).astype(np.int64)
            marg = (np.abs(u[k] - np.round(u[k])) < 1e-4) | (np.abs(v[k] - np.round(v[k])) < 1e-4)   # (pixels; fp32 u, v of ~1e3 carry ~1e-4)
            cand_p.append(py * W + px); cand_z.append(h[k, 2]); cand_ord.append(order_base + idx[k]); cand_m.append(np.full(len(k), i))
            cand_q.append(np.where(marg, 1.0, 0.0)); cand_c.append(col[k]); cand_cos.append(np.ones(len(k)))
        else:
            nrm = s[:, 8:11] @ M[:3, :3].T
            r = s[:, 11]
            # quad corners in the model frame (draw_global_surface.geom), projected: the candidate pixels
            nm = s[:, 8:11]
            ax = np.stack([nm[:, 1] - nm[:, 2], -nm[:, 0], nm[:, 0]], 1)
            al = np.linalg.norm(ax, axis=1)
            good = al > 0
            ax = ax / np.where(good, al, 1.0)[:, None] * (r * np.sqrt(2.0))[:, None]
            ay = np.cross(nm, ax)
            corners = [s[:, :3] + ax, s[:, :3] + ay, s[:, :3] - ay, s[:, :3] - ax]
            cz = np.stack([c @ M[2, :3] + M[2, 3] for c in corners], 1)
            cxs = np.stack([c @ M[0, :3] + M[0, 3] for c in corners], 1)
            cys = np.stack([c @ M[1, :3] + M[1, 3] for c in corners], 1)
            behind = (cz < near).sum(1)
            beyond = (cz > far).sum(1)
            good &= (behind < 4) & (beyond < 4)
            with np.errstate(divide="ignore", invalid="ignore"):
                us, vs = fx * cxs / cz + cx, fy * cys / cz + cy
            x0 = np.where(behind > 0, 0, np.floor(np.nan_to_num(us.min(1), nan=0) - 0.5) - 1)
            x1 = np.where(behind > 0, W - 1, np.floor(np.nan_to_num(us.max(1), nan=W) - 0.5) + 1)
            y0 = np.where(behind > 0, 0, np.floor(np.nan_to_num(vs.min(1), nan=0) - 0.5) - 1)
            y1 = np.where(behind > 0, H - 1, np.floor(np.nan_to_num(vs.max(1), nan=H) - 0.5) + 1)
            x0, x1 = np.clip(x0, 0, W).astype(np.int64), np.clip(x1, -1, W - 1).astype(np.int64)
            y0, y1 = np.clip(y0, 0, H).astype(np.int64), np.clip(y1, -1, H - 1).astype(np.int64)
            good &= (x0 <= x1) & (y0 <= y1)
            k = np.nonzero(good)[0]
            bw, bh = x1[k] - x0[k] + 1, y1[k] - y0[k] + 1
            cnt = bw * bh
            rep = np.repeat(np.arange(len(k)), cnt)
            off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            j = k[rep]
            px = x0[j] + off % bw[rep]
            py = y0[j] + off // bw[rep]
            lx = (px + 0.5 - cx) / fx
            ly = (py + 0.5 - cy) / fy
            nj = nrm[j]
            hj = h[j]
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (hj * nj).sum(1) / (lx * nj[:, 0] + ly * nj[:, 1] + nj[:, 2])
                d = np.stack([lx * t, ly * t, t], 1) - hj
                q = (d * d).sum(1) / (r[j] ** 2)
            inside = (q <= 1.0) & (t >= near) & (t <= far)
            # (a winner whose ray grazes its disc, |cos| < 0.02, meets the plane at a depth fp32 cannot pin to 1e-5: ambiguous, below)
            # (the rim margin also covers fp32's cancellation in hit - centre: about two ulps of |centre|, 2.5e-7 |h|, against a radius of ~1 cm)
            cosang = np.abs(lx * nj[:, 0] + ly * nj[:, 1] + nj[:, 2]) / np.sqrt((lx * lx + ly * ly + 1.0) * (nj * nj).sum(1))
            # (... and the hit's own error, which grows as 1 / cos when the ray grazes the disc)
            rim = np.abs(np.sqrt(np.maximum(q, 0.0)) - 1.0) * r[j] < (EPS * r[j] + 2.5e-7 * np.linalg.norm(hj, axis=1)
                                                                     + GRAZE * np.abs(t) * np.sqrt(lx * lx + ly * ly + 1.0) / np.maximum(cosang, 1e-6))
            marg = rim | (np.abs(t - near) < EPS * near) | (np.abs(t - far) < EPS * far)
            sel = inside | marg
            cand_p.append(py[sel] * W + px[sel]); cand_z.append(t[sel]); cand_ord.append(order_base + idx[j[sel]])
            cand_m.append(np.full(int(sel.sum()), i)); cand_q.append(np.where(marg[sel], 1.0, 0.0) + np.where(inside[sel], 0.0, 2.0))
            cand_c.append(col[j[sel]]); cand_cos.append(cosang[sel])
        order_base += 1 << 40
    rgba = np.empty((H, W, 4), np.uint8)
    rgba[:] = np.array(view.clear_rgba[:], np.uint8)
    depth = np.zeros((H, W), np.float64)
    model = np.full((H, W), -1, np.int32)
    amb = np.zeros((H, W), bool)
    if not cand_p:
        return rgba, depth, model, amb
    p = np.concatenate(cand_p); z = np.concatenate(cand_z); o = np.concatenate(cand_ord); mi = np.concatenate(cand_m)
    flag = np.concatenate(cand_q); c = np.concatenate(cand_c) if cand_c else np.zeros((0, 3))
    inside = flag < 2
    marginal = (flag == 1) | (flag == 3)
    # winners among the covering candidates: smallest z, then the first drawn
    ins = np.nonzero(inside)[0]
    srt = ins[np.lexsort((o[ins], z[ins], p[ins]))]
    first = np.ones(len(srt), bool)
    first[1:] = p[srt][1:] != p[srt][:-1]
    win = srt[first]
    pw = p[win]
    rgba.reshape(-1, 4)[pw, :3] = np.floor(np.clip(c[win], 0, 1) * 255.0 + 0.5).astype(np.uint8)
    rgba.reshape(-1, 4)[pw, 3] = 255
    depth.reshape(-1)[pw] = z[win]
    model.reshape(-1)[pw] = mi[win]
    # ambiguity: a runner-up within EPS, or a marginal candidate that could take the pixel -- when it would draw something else (coplanar
    # surfels of one fused surface meet a ray at the same depth all the time; which of two equal results -- colour, model, depth to 1e-5 -- wins
    # does not matter)
    c8 = np.floor(np.clip(c, 0, 1) * 255.0 + 0.5)
    w_of = np.full(H * W, -1, np.int64)
    w_of[pw] = win

    def differs(k):
        w = w_of[p[k]]
        w0 = np.maximum(w, 0)
        return (w < 0) | (np.abs(c8[k] - c8[w0]).max(1) > 1) | (mi[k] != mi[w0]) | (np.abs(z[k] - z[w0]) > EPS * np.abs(z[w0]))
    cs = np.concatenate(cand_cos)
    unc = DEPTH_EPS + GRAZE / np.maximum(cs, 1e-6)
    others = np.nonzero(inside)[0]
    wk = w_of[p[others]]
    others, wk = others[(wk >= 0) & (wk != others)], wk[(wk >= 0) & (wk != others)]
    close = z[others] <= z[wk] * (1.0 + unc[others] + unc[wk])
    amb.reshape(-1)[p[others][close & differs(others)]] = True
    best = np.full(H * W, np.inf)
    best[pw] = z[win]
    mk = np.nonzero(marginal)[0]
    could = z[mk] <= best[p[mk]] * (1 + EPS)
    is_win = w_of[p[mk]] == mk
    amb.reshape(-1)[p[mk][could & (is_win | differs(mk))]] = True
    amb.reshape(-1)[pw[cs[win] < 0.02]] = True
    return rgba, depth, model, amb
