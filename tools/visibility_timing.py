"""Times the cloud visibility kernel (mf_cloud_visibility_dev; maskfusion_amd/csrc/mf_eval_visibility.hip) at the size it was written for: the
26.9 M points of a dense room map (synth.dense_room_map, the targets of tools/eval_timing.py) against 32 frames of synth.Stream at 640 x 480
with the stream's own poses, tolerance 5 cm.

  one call     all 32 frames in one call, points as xyz (stride 3) and as the map's own records (stride 12)
  chunks       the same frames as two calls of 16 with accumulate, what eval.observe_sequence issues
  bytes        what a perfect gather would move: every point read once, one depth sample per point and frame in whose frustum the point is,
               the poses, and one row of outputs written per point -- and the rate that is of the measured time
  numpy        the restatement of the rule (tests/visibility_restatement.py) on every 100th point, for scale

Device times are medians of 20 calls after 5 warm-up calls, between HIP events on the call's stream.  Prints one JSON line at the end.

    python tools/visibility_timing.py [--points 26.9e6] [--frames 32] [--every 8] [--no-numpy]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, stream, reps=20, warm=5):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(min(out)), float(max(out))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=float, default=26.9e6)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--every", type=int, default=8, help="the stream's frame k * EVERY is the k-th depth frame")
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args(argv)
    import torch
    from maskfusion_amd import eval as ev
    from maskfusion_amd import synth
    from maskfusion_amd.lib import load
    L = load()
    t0 = time.perf_counter()
    st = synth.Stream()
    room = synth.dense_room_map(st.scene, int(a.points), last_time=1.0)
    ids = [k * a.every for k in range(a.frames)]
    depth = np.stack([st.frame(k)[1] for k in ids])
    cam = ev.cam_from_cloud(np.stack([st.gt_pose(k) for k in ids]))
    n, F = len(room), a.frames
    print(f"{n} points, {F} frames of {st.W} x {st.H} (generated in {time.perf_counter() - t0:.1f} s)")
    K = (st.fx, st.fy, st.cx, st.cy)
    rule = (0.01, float(np.finfo(np.float32).max), 0.05, 0.0)
    d_rec = torch.from_numpy(room).cuda()
    d_xyz = d_rec[:, :3].contiguous()
    d_depth, d_cam = torch.from_numpy(depth).cuda(), torch.from_numpy(cam).cuda()
    counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    first = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()

    def call(points, f0, f1, accumulate):
        rc = L.mf_cloud_visibility_dev(points.data_ptr(), int(points.shape[1]), n, d_depth[f0:f1].data_ptr(), d_cam[f0:f1].data_ptr(), f1 - f0, st.H, st.W, *K,
                                       *rule, f0, accumulate, counts.data_ptr(), first.data_ptr(), stream.cuda_stream)
        assert rc == 0, rc

    res = {"points": n, "frames": F, "width": st.W, "height": st.H}
    for name, pts in (("stride3", d_xyz), ("stride12", d_rec)):
        med, lo, hi = _median_ms(lambda: call(pts, 0, F, 0), stream)
        res[name + "_ms"] = med
        res[name + "_point_frames_per_s"] = n * F / (med * 1e-3)
        print(f"one call, {name}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}), {n * F / (med * 1e-3):.3e} point-frames/s")
    whole = counts.cpu().numpy().view(np.uint32).copy()
    half = F // 2

    def chunks():
        call(d_xyz, 0, half, 0)
        call(d_xyz, half, F, 1)
    med, lo, hi = _median_ms(chunks, stream)
    res["two_chunks_ms"] = med
    print(f"two chunks of {half}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), whole), "the chunked result differs from the single call's"
    in_frustum = int(whole[:, 0].astype(np.int64).sum())
    ideal = n * 12 + in_frustum * 4 + F * 48 + n * 20
    res.update(in_frustum_point_frames=in_frustum, perfect_gather_bytes=ideal, perfect_gather_GBps_stride3=ideal / (res["stride3_ms"] * 1e-3) / 1e9)
    keep = ev.observed(whole)
    res["summary"] = ev.visibility_summary(whole, keep, F)
    print(f"in-frustum point-frames {in_frustum} of {n * F}; a perfect gather moves {ideal / 1e6:.1f} MB: {res['perfect_gather_GBps_stride3']:.0f} GB/s of the "
          f"measured time; summary {res['summary']}")
    if not a.no_numpy:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import visibility_restatement as vr
        sample = np.ascontiguousarray(room[::100, :3])
        t0 = time.perf_counter()
        c, _ = vr.visibility(sample, depth, cam, *K, *rule)
        dt = time.perf_counter() - t0
        assert np.array_equal(c, whole[::100]), "the restatement differs from the device on the sample"
        res.update(numpy_sample_points=len(sample), numpy_sample_s=dt, numpy_point_frames_per_s=len(sample) * F / dt)
        print(f"numpy restatement on {len(sample)} points: {dt:.2f} s, {len(sample) * F / dt:.3e} point-frames/s (equal to the device on the sample)")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
