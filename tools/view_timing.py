"""Times the view score (mf_view_score_dev) on the MI355X beside the render it compares (mf_render_view_dev from the sensor's view), for one
640 x 480 frame: the median of 20 calls after 5 warm-up calls, HIP events on the context's stream.  DESIGN.md "View evaluation" quotes it.

    python tools/view_timing.py

The frame: the S2 VGA scene (two tracked boxes) after 12 frames, as tools/render_timing.py uses it.  The score is timed with the groups
ViewScorer.add_from derives (one per model) and with a single group and no group image.  A measurement needs the GPU: there is no fallback."""
from __future__ import annotations

import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(stream, call, sync, reps=20, warmup=5):
    import torch
    for _ in range(warmup):
        call()
    sync()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)   # torch's HIP context first
    from maskfusion_amd import MaskFusion, synth
    from maskfusion_amd import eval as ev
    from maskfusion_amd.lib import load
    W, H = 640, 480
    st = synth.Stream(W=W, H=H, fx=528.0, fy=528.0, cx=320.0, cy=240.0, n_objects=2, noise=True, object_motion=1.0)
    mf = MaskFusion(W, H, 528.0, 528.0, 320.0, 240.0, icpThresh=100.0, so3=False, numGSurfels=1 << 20, numOSurfels=1 << 18, enableMultipleModels=True,
                    modelSpawnOffset=3, trackAllModels=True)
    for k, v in (("mfThreshold", 0.3), ("mfWeightDistance", 150.0), ("mfWeightConvexity", 2.8), ("mfMorphEdgeIterations", 0), ("mfMorphMaskIterations", 0),
                 ("newModelMinRelativeSize", 0.004)):
        mf.setParam(k, v)
    for k in range(12):
        rgb, depth, mask = st.frame(k)
        mf.processFrame(rgb, depth, mask=mask, classIDs=[0, 41, 42], timestamp=k)
    view = mf.sensorRenderView()
    s = torch.cuda.ExternalStream(mf.stream(), device=dev)
    r = torch.empty((1, H, W, 4), dtype=torch.uint8, device=dev)
    rd = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    mod = torch.empty((1, H, W), dtype=torch.int32, device=dev)
    c, d = torch.as_tensor(rgb[None]).to(dev), torch.as_tensor(depth[None]).to(dev)
    render = lambda: mf.renderViewDevice(view, r.data_ptr(), rd.data_ptr(), mod.data_ptr())
    render()
    mf.sync()
    g = (mod + 1).to(torch.uint8).contiguous()        # one group per model, 0: nothing drawn
    torch.cuda.synchronize()
    L = load()
    out = torch.empty((1, 64, 10), dtype=torch.int64, device=dev)

    def score(group, n):
        rc = L.mf_view_score_dev(r.data_ptr(), rd.data_ptr(), c.data_ptr(), d.data_ptr(), group.data_ptr() if group is not None else None, 1, H, W, n,
                                 float(np.finfo(np.float32).max), 0.01, out.data_ptr(), mf.stream())
        assert rc == 0, rc

    models = len(mf.getModels())
    t_render = timed(s, render, mf.sync)
    t_groups = timed(s, lambda: score(g, 64), mf.sync)
    t_single = timed(s, lambda: score(None, 1), mf.sync)
    score(g, 64)
    mf.sync()
    m = ev.view_metrics(out.cpu().numpy().view(np.uint64))["summary"]
    fmt = lambda t: f"{t[0]:.1f} us (median of 20; {t[1]:.1f} .. {t[2]:.1f})"
    print(f"{W}x{H}, {models} models, sensor view: mf_render_view_dev {fmt(t_render)}; mf_view_score_dev, 64 groups with a group image {fmt(t_groups)}; "
          f"one group, no group image {fmt(t_single)} (each with its memset of the counters)", flush=True)
    print("the frame's scores:", {k: m[k] for k in ev.VIEW_KEYS}, flush=True)
    mf.close()


if __name__ == "__main__":
    main()
