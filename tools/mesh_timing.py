"""Times the surfel meshing (mf_cloud_mesh_build_dev / mf_cloud_mesh_emit_dev; maskfusion_amd/csrc/mf_mesh.hip) at configs[4] size: a dense room
map of 26.9 M surfels (synth.dense_room_map, the background of stress.make_context's scenario) with its normals and decoded colours, meshed
at a 1 cm voxel with the default support of 2.5 voxels on the lattice maskfusion_amd.mesh.lattice_for derives.

Per stage, the device time between HIP events on the call's stream, as the build itself records them (stage_ms of
mf_cloud_mesh_build_dev; stage 2 is the host's: the wait for the block count, its read-back and the allocation), and the emit between
events around the call; medians of --reps calls after one warm-up.  A report: nothing is gated on a time.

    python tools/mesh_timing.py [--points 26.9e6] [--voxel 0.01] [--support-voxels 2.5] [--reps 3] [--out profiles/mesh_timing.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ["eligible points, normals, block marks, directory scan", "grid build", "host: wait, block count, allocation", "block list + field",
          "cells + quads", "vertex and quad scans"]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=float, default=26.9e6)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--support-voxels", type=float, default=2.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from maskfusion_amd import mesh as M
    from maskfusion_amd import stress, synth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    st = stress.stream()
    room = synth.dense_room_map(st.scene, int(a.points), last_time=1.0, furniture_above=st.masked_objects)
    col = room[:, 4].astype(np.int64)
    rec = np.empty((len(room), 9), np.float32)
    rec[:, :3], rec[:, 3:6] = room[:, :3], -room[:, 8:11]
    rec[:, 6], rec[:, 7], rec[:, 8] = col >> 16 & 0xFF, col >> 8 & 0xFF, col & 0xFF
    support = a.support_voxels * a.voxel
    d = torch.from_numpy(rec).cuda()
    origin, dims = M.lattice_for(d[:, :3], d[:, 3:6], a.voxel, support)
    say(f"cloud: {len(rec)} surfels (generated in {time.perf_counter() - t0:.1f} s); voxel {a.voxel} m, support {support:g} m, lattice "
        f"{dims[0]} x {dims[1]} x {dims[2]} corners = {int(np.prod(dims.astype(np.int64))) / 1e6:.0f} M, "
        f"{int(np.prod((dims.astype(np.int64) + 7) // 8))} blocks in the directory")
    s = torch.cuda.current_stream()
    builds, emits, wall = [], [], []
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        m = M.Mesh(d, 3, 6, origin, a.voxel, dims, support, 3, stage_ms=True)
        t_build = time.perf_counter() - t0
        held = free0 - torch.cuda.mem_get_info()[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        out = m.emit(cells=True)
        e1.record(s)
        e1.synchronize()
        if rep:
            builds.append(m.stage_ms.copy()); emits.append(e0.elapsed_time(e1)); wall.append(t_build * 1e3)
        nv, nq = m.n_vertices, m.n_quads
        del out
        m.close()
    b = np.median(np.array(builds), 0)
    say(f"mesh: {nv} vertices, {nq} quads ({2 * nq} triangles); the handle holds {held / 2**20:.0f} MiB")
    for name, ms in zip(STAGES, b):
        say(f"  {name:55s} {ms:9.2f} ms")
    say(f"  {'emit (vertices, normals, colours, cells, quads)':55s} {float(np.median(emits)):9.2f} ms")
    say(f"build, wall clock of the call: median {float(np.median(wall)):.1f} ms over {a.reps} calls; device stages {float(b.sum()):.1f} ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
