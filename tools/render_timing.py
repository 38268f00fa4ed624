"""Times the headless render (mf_render_view_dev) on the MI355X: the median of 20 calls after 5 warm-up calls, HIP events on the context's
stream, beside the same frame's prediction pair (passTimings bgPredict + objPredict).

    python tools/render_timing.py [--skip-c4]

Cases: the S2 VGA scene (640 x 480, two tracked boxes) rendered at 640 x 480 and 1280 x 980 from the follow view; the configs[4] dense scenario
(maskfusion_amd/stress.py, 1280 x 960) from the camera's own view (its intrinsics, the current pose) and from the follow view.  For every case
one line: the surfels of the drawn models (what the cull may visit; the run table lets it skip most of them), the algorithmic bytes (48 B per
such surfel + the output image) and that figure / 8 TB/s.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_render(mf, view, reps=20, warmup=5):
    import torch
    dev = torch.device("cuda", 0)
    H, W = int(view.height), int(view.width)
    d_rgba = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    d_dep = torch.empty((H, W), dtype=torch.float32, device=dev)
    d_mod = torch.empty((H, W), dtype=torch.int32, device=dev)
    s = torch.cuda.ExternalStream(mf.stream(), device=dev)
    for _ in range(warmup):
        mf.renderViewDevice(view, d_rgba.data_ptr(), d_dep.data_ptr(), d_mod.data_ptr())
    mf.sync()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        mf.renderViewDevice(view, d_rgba.data_ptr(), d_dep.data_ptr(), d_mod.data_ptr())
        b.record(s)
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    drawn = int((d_mod >= 0).sum().item())
    return statistics.median(ts), drawn


def report(name, mf, view, predict_us):
    us, drawn = time_render(mf, view)
    surfels = sum(m.lastCount() for m in mf.getModels())
    out_bytes = int(view.width) * int(view.height) * (4 + 4 + 4)
    algo = 48 * surfels + out_bytes
    print(f"{name}: {int(view.width)}x{int(view.height)} render {us:.1f} us (median of 20); surfels of the drawn models {surfels}; pixels drawn {drawn}; "
          f"algorithmic bytes {algo / 1e6:.1f} MB -> {algo / 8e12 * 1e6:.1f} us at 8 TB/s; same frame's bgPredict + objPredict {predict_us:.1f} us "
          f"(render / prediction {us / max(predict_us, 1e-9):.2f})", flush=True)


def s2_case():
    from maskfusion_amd import MaskFusion, synth
    st = synth.Stream(W=640, H=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, n_objects=2, noise=True, object_motion=1.0)
    mf = MaskFusion(640, 480, 528.0, 528.0, 320.0, 240.0, icpThresh=100.0, so3=False, numGSurfels=1 << 20, numOSurfels=1 << 18, enableMultipleModels=True,
                    modelSpawnOffset=3, trackAllModels=True)
    for k, v in (("mfThreshold", 0.3), ("mfWeightDistance", 150.0), ("mfWeightConvexity", 2.8), ("mfMorphEdgeIterations", 0), ("mfMorphMaskIterations", 0),
                 ("newModelMinRelativeSize", 0.004)):
        mf.setParam(k, v)
    mf.setParam("passTimings", 1)
    for k in range(12):
        rgb, depth, mask = st.frame(k)
        mf.processFrame(rgb, depth, mask=mask, classIDs=[0, 41, 42], timestamp=k)
    pt = mf.passTimings()
    pred = (pt["bgPredict"] + pt["objPredict"]) * 1e3
    for (w, h) in ((640, 480), (1280, 980)):
        report(f"S2 follow view ({len(mf.getModels())} models)", mf, mf.defaultRenderView(w, h), pred)
    v = mf.defaultRenderView(640, 480)
    v.fx, v.fy = 528.0, 528.0
    report("S2 camera view", mf, v, pred)
    mf.close()


def c4_case():
    from maskfusion_amd import stress
    st = stress.stream(4)
    cls = [0] + [41 + i for i in range(4)]
    mf = stress.make_context(0)
    frames = [st.frame(k) for k in range(14)]
    k0, _ = stress.lead_in(mf, st, frames, cls, n_objects=4, max_frames=10)
    mf.setParam("passTimings", 1)
    for k in range(k0, k0 + 2):
        rgb, depth, mask = frames[k]
        mf.processFrame(rgb, depth, mask=mask, classIDs=cls, timestamp=k)
    pt = mf.passTimings()
    pred = (pt["bgPredict"] + pt["objPredict"]) * 1e3
    v = mf.defaultRenderView(stress.W, stress.H)
    v.fx = v.fy = stress.F
    v.cx, v.cy = stress.W / 2.0, stress.H / 2.0
    v.set_pose(mf.getCurrPose())
    report("configs[4] camera view", mf, v, pred)
    report("configs[4] follow view", mf, mf.defaultRenderView(stress.W, stress.H), pred)
    mf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-c4", action="store_true")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")   # torch's HIP context first (torch created after the library's finds no device here)
    s2_case()
    if not a.skip_c4:
        c4_case()


if __name__ == "__main__":
    main()
