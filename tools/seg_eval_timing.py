"""Times the two device calls behind the segmentation scores (mf_label_confusion_dev, mf_label_boundary_dev) on the benchmark's size --
600 frames of 640 x 480 with 8 objects, radius 6 -- and, beside them, a numpy / scipy.ndimage computation of the same counts on 16
processes.  Prints one JSON line; --out FILE also writes it there (profiles/seg_eval_timing.json is the copy DESIGN.md quotes).

    python tools/seg_eval_timing.py [--frames 600] [--distinct 30] [--host-frames 600] [--out FILE]

Labels: the instance masks synth.Scene renders along the benchmark's camera path; frame k's ground truth is view k % distinct, its estimate
view k % distinct + 1 (the next camera position: every object a few pixels off).  --distinct bounds the rendering time; the counts do
not care that views repeat.  The device times are medians of 20 calls after 5 warm-ups, each call timed by a host clock around the call
and a device synchronise (the result stays on the device).  The host computation runs FIRST, in worker processes that never touch the GPU,
and the tool checks that both give the same counts.  A measurement needs the GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N_OBJECTS, RADIUS = 640, 480, 8, 6
_G = {}


def _disc(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return xx * xx + yy * yy <= r * r


def _boundary(cls, k):
    mine = cls == k
    other = np.zeros_like(mine)
    other[:, 1:] |= cls[:, :-1] != cls[:, 1:]
    other[:, :-1] |= cls[:, 1:] != cls[:, :-1]
    other[1:, :] |= cls[:-1, :] != cls[1:, :]
    other[:-1, :] |= cls[1:, :] != cls[:-1, :]
    return mine & other


def _host_frame(f):
    """the region and boundary counts of frame f with numpy and one scipy.ndimage dilation per object and side"""
    from scipy import ndimage
    views, distinct, n = _G["views"], _G["distinct"], N_OBJECTS + 1
    gt, est = views[f % distinct].astype(np.int64), views[f % distinct + 1].astype(np.int64)
    counts = np.bincount((gt * n + est).reshape(-1), minlength=n * n).reshape(n, n)
    rows = np.zeros((n, 4), np.int64)
    disc = _disc(RADIUS)
    for k in range(n):
        be, bg = _boundary(est, k), _boundary(gt, k)
        rows[k] = (be.sum(), (be & ndimage.binary_dilation(bg, disc)).sum(), bg.sum(), (bg & ndimage.binary_dilation(be, disc)).sum())
    return counts, rows


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--distinct", type=int, default=30, help="rendered views (the stream cycles through them)")
    ap.add_argument("--host-frames", type=int, default=600, help="frames the host computation covers (its time is scaled to --frames)")
    ap.add_argument("--processes", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    from maskfusion_amd import synth
    st = synth.Stream(W=W, H=H, n_objects=N_OBJECTS, noise=False)
    t0 = time.time()
    views = np.stack([st.frame(k)[2] for k in range(a.distinct + 1)]).astype(np.uint8)
    render_s = time.time() - t0
    _G.update(views=views, distinct=a.distinct)

    # the host computation: before this process opens the GPU
    import multiprocessing as mp
    hf = min(a.host_frames, a.frames)
    with mp.get_context("fork").Pool(a.processes) as pool:
        pool.map(_host_frame, range(min(hf, a.processes)))              # the workers import scipy
        t0 = time.time()
        host = pool.map(_host_frame, range(hf), chunksize=max(1, hf // (4 * a.processes)))
        host_s = time.time() - t0

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("seg_eval_timing: no GPU visible; the device calls cannot be timed here\n")
        return 2
    from maskfusion_amd import eval as ev
    from maskfusion_amd.lib import load
    L = load()
    idx = np.arange(a.frames) % a.distinct
    dv = torch.from_numpy(views).cuda()
    gt = dv[torch.from_numpy(idx).cuda()].contiguous()
    est = dv[torch.from_numpy(idx + 1).cuda()].contiguous()
    n = N_OBJECTS + 1
    lut = np.full(256, 255, np.uint8)
    lut[:n] = np.arange(n)
    pair = np.arange(n, dtype=np.uint8)
    counts = torch.zeros((a.frames, n, n), dtype=torch.int32, device="cuda")
    rows = torch.zeros((a.frames, n, 4), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def conf():
        return L.mf_label_confusion_dev(est.data_ptr(), gt.data_ptr(), a.frames, H, W, lut.ctypes.data, n, lut.ctypes.data, n, counts.data_ptr(), stream)

    def bnd():
        return L.mf_label_boundary_dev(est.data_ptr(), gt.data_ptr(), a.frames, H, W, lut.ctypes.data, n, lut.ctypes.data, n, pair.ctypes.data, RADIUS,
                                       rows.data_ptr(), stream)

    def median_ms(call):
        ts = []
        for k in range(25):
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc = call()
            torch.cuda.synchronize()
            if rc != 0:
                raise RuntimeError(f"the device call failed with code {rc}")
            if k >= 5:
                ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    conf_ms, bnd_ms = median_ms(conf), median_ms(bnd)
    c, r = counts.cpu().numpy(), rows.cpu().numpy()
    same = all(np.array_equal(c[f], host[f][0]) and np.array_equal(r[f], host[f][1]) for f in range(hf))
    pixels = a.frames * W * H
    boundary_share = float((r[:, :, 0].sum() + r[:, :, 2].sum()) / (2.0 * pixels))
    out = {"tool": "seg_eval_timing", "device": torch.cuda.get_device_name(0), "frames": a.frames, "width": W, "height": H, "objects": N_OBJECTS,
           "radius": RADIUS, "distinct_views": a.distinct, "render_s": render_s,
           "confusion_ms": {"median": conf_ms[0], "min": conf_ms[1], "max": conf_ms[2]},
           "confusion_read_bytes": 2 * pixels, "confusion_gbytes_per_s": 2 * pixels / (conf_ms[0] * 1e-3) / 1e9,
           "boundary_ms": {"median": bnd_ms[0], "min": bnd_ms[1], "max": bnd_ms[2]}, "boundary_pixel_share": boundary_share,
           "host_processes": a.processes, "host_frames": hf, "host_s": host_s, "host_s_scaled_to_all_frames": host_s * a.frames / hf,
           "host_counts_equal_device_counts": bool(same)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
