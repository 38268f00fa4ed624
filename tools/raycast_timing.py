"""Times the mesh rendering (mf_trimesh_render_dev; maskfusion_amd/csrc/mf_trimesh_ray.hip) at configs[4] size: the surface-nets mesh of the
dense room map as tools/trimesh_timing.py builds it (about 1.67 M triangles, cell 0.025 m), rendered at 640 x 480 and at 1280 x 960 from
three poses of the synthetic stream's camera.

Between HIP events on the call's stream, medians of --reps calls after one warm-up per pose and size.  The call synchronises its stream
before it returns, so the events enclose the whole kernel.  A report: nothing is gated on a time.

    python tools/raycast_timing.py [--points 26.9e6] [--cell 0.025] [--reps 3] [--out profiles/raycast_timing.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=float, default=26.9e6)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--cell", type=float, default=0.025)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", default="0,45,90", help="the stream's frames whose camera poses are rendered")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from maskfusion_amd import eval as ev
    from maskfusion_amd import mesh as M
    from maskfusion_amd import stress, synth
    from maskfusion_amd.lib import load
    L = load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    st = stress.stream()
    room = synth.dense_room_map(st.scene, int(a.points), last_time=1.0, furniture_above=st.masked_objects)
    pts = torch.from_numpy(np.ascontiguousarray(room[:, :3])).cuda()
    nrm = torch.from_numpy(np.ascontiguousarray(-room[:, 8:11])).cuda()
    v, _, _, tri = M.mesh_cloud(pts, nrm, None, voxel=a.voxel)
    del pts, nrm, room
    torch.cuda.empty_cache()
    say(f"mesh: {len(v)} vertices, {len(tri)} triangles (surface nets of {int(a.points)} surfels at a {a.voxel} m voxel); cell {a.cell} m "
        f"(set up in {time.perf_counter() - t0:.1f} s)")
    dv, dt = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (v, tri))
    s = torch.cuda.current_stream()
    stream = s.cuda_stream
    h, ne = C.c_void_p(), C.c_uint32(0)
    if L.mf_trimesh_build_dev(dv.data_ptr(), 3, len(v), dt.data_ptr(), len(tri), a.cell, C.byref(h), C.byref(ne), stream) != 0:
        raise SystemExit("mf_trimesh_build_dev: " + L.mf_last_error(None).decode())
    poses = [synth.camera_pose(int(k)) for k in a.frames.split(",")]
    inf = float("inf")
    for W, H in ((640, 480), (1280, 960)):
        fx, fy, cx, cy = 528.0 * W / 640, 528.0 * H / 480, 320.0 * W / 640, 240.0 * H / 480
        depth = torch.empty(W * H, dtype=torch.float32, device="cuda")
        idx = torch.empty(W * H, dtype=torch.int32, device="cuda")
        uv = torch.empty((W * H, 2), dtype=torch.float32, device="cuda")
        front = torch.empty(W * H, dtype=torch.uint8, device="cuda")
        per_pose = []
        for k, T in zip(a.frames.split(","), poses):
            T16 = ev._pack_T(T)
            ms = []
            for rep in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                rc = L.mf_trimesh_render_dev(h, W, H, fx, fy, cx, cy, T16.ctypes.data, 0.0, inf, depth.data_ptr(), idx.data_ptr(), uv.data_ptr(), front.data_ptr(), stream)
                e1.record(s)
                e1.synchronize()
                if rc != 0:
                    raise SystemExit("mf_trimesh_render_dev: " + L.mf_last_error(None).decode())
                if rep:
                    ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            per_pose.append(med)
            hit = idx >= 0
            d = depth[hit].double()
            say(f"  {W} x {H}, pose of frame {k:>3s}: {med:8.3f} ms   {W * H / med / 1e3:8.1f} M rays / s   {int(hit.sum())} of {W * H} pixels hit, "
                f"mean depth {float(d.mean()) if len(d) else 0.0:.3f} m, front {int(front[hit].sum())}")
        say(f"  {W} x {H}: median of the poses {float(np.median(per_pose)):.3f} ms per frame, {W * H / float(np.median(per_pose)) / 1e3:.1f} M rays / s")
    L.mf_trimesh_free(h)
    say(f"medians of {a.reps} calls after one warm-up, between HIP events on the call's stream")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
