"""Times the mesh evaluation (mf_trimesh_*; maskfusion_amd/csrc/mf_eval_trimesh.hip) at configs[4] size: the surface-nets mesh of the dense room
map as tools/mesh_timing.py builds it (about 1.67 M triangles), queried with 5 M jittered surfels of that map at radius 0.05 m and cell
0.025 m.

Between HIP events on the calls' stream, medians of --reps calls after one warm-up: the build (its host wait for the pair count and its
allocation included), the query, and the sample plan plus emit at density 10 000 per square metre.  Beside these, mf_cloud_nn_dev of the
same queries against the mesh's vertex cloud: the approximation a user had before.  A report: nothing is gated on a time.

    python tools/trimesh_timing.py [--points 26.9e6] [--queries 5e6] [--radius 0.05] [--cell 0.025] [--density 10000] [--reps 3] [--out profiles/trimesh_timing.txt]
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
    ap.add_argument("--queries", type=float, default=5e6)
    ap.add_argument("--jitter", type=float, default=0.005, help="sigma of the queries' offset from their surfels, metres")
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--cell", type=float, default=0.025)
    ap.add_argument("--density", type=float, default=10000.0)
    ap.add_argument("--reps", type=int, default=3)
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
    rng = np.random.default_rng(0)
    pick = rng.choice(len(room), int(a.queries), replace=False)
    q = (room[pick, :3] + rng.normal(scale=a.jitter, size=(len(pick), 3))).astype(np.float32)
    del pts, nrm, room
    torch.cuda.empty_cache()
    say(f"mesh: {len(v)} vertices, {len(tri)} triangles (surface nets of {int(a.points)} surfels at a {a.voxel} m voxel); {len(q)} queries, jitter "
        f"{a.jitter} m; radius {a.radius} m, cell {a.cell} m, density {a.density:g} / m^2 (set up in {time.perf_counter() - t0:.1f} s)")
    dv, dt, dq = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (v, tri, q))     # (quads_to_triangles hands back a strided view)
    nq = len(q)
    dist = torch.empty(nq, dtype=torch.float32, device="cuda")
    idx = torch.empty(nq, dtype=torch.int32, device="cuda")
    closest = torch.empty((nq, 3), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    stream = s.cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        out = fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def check(rc, name):
        if rc != 0:
            raise SystemExit(f"{name} failed with code {rc}: {L.mf_last_error(None).decode()}")

    t_build, t_query, t_sample, t_nn = [], [], [], []
    ws, need = ev._workspace(L, "mf_cloud_nn_workspace", dq.device, len(v))
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        h, ne, ns = C.c_void_p(), C.c_uint32(0), C.c_uint64(0)
        ms_b, rc = timed(lambda: L.mf_trimesh_build_dev(dv.data_ptr(), 3, len(v), dt.data_ptr(), len(tri), a.cell, C.byref(h), C.byref(ne), stream))
        check(rc, "mf_trimesh_build_dev")
        held = free0 - torch.cuda.mem_get_info()[0]
        ms_q, rc = timed(lambda: L.mf_trimesh_distance_dev(h, dq.data_ptr(), 3, nq, None, a.radius, dist.data_ptr(), idx.data_ptr(), closest.data_ptr(), stream))
        check(rc, "mf_trimesh_distance_dev")

        def plan_and_emit():
            rc = L.mf_trimesh_sample_plan_dev(h, a.density, C.byref(ns), stream)
            if rc != 0:
                return rc, None
            p = torch.empty((max(int(ns.value), 1), 3), dtype=torch.float32, device="cuda")
            n = torch.empty_like(p)
            return L.mf_trimesh_sample_emit_dev(h, p.data_ptr(), n.data_ptr(), None, stream), p
        ms_s, (rc, _) = timed(plan_and_emit)
        check(rc, "mf_trimesh_sample_*")
        L.mf_trimesh_free(h)
        if rep == a.reps:
            hits = int((idx >= 0).sum())
            d = dist[idx >= 0].double()
            say(f"triangles: {ne.value} of {len(tri)} eligible; the handle holds {held / 2**20:.0f} MiB; {ns.value} samples")
            say(f"queries: {hits} of {nq} within the radius; distance mean {float(d.mean()) * 1e3:.3f} mm, median {float(d.median()) * 1e3:.3f} mm")
        ms_n, rc = timed(lambda: L.mf_cloud_nn_dev(dv.data_ptr(), 3, len(v), dq.data_ptr(), 3, nq, None, a.radius, dist.data_ptr(), idx.data_ptr(), ws.data_ptr(), need, stream))
        check(rc, "mf_cloud_nn_dev")
        if rep == a.reps:
            d = dist[idx >= 0].double()
            say(f"nearest VERTEX of the same queries: distance mean {float(d.mean()) * 1e3:.3f} mm, median {float(d.median()) * 1e3:.3f} mm")
        if rep:
            t_build.append(ms_b); t_query.append(ms_q); t_sample.append(ms_s); t_nn.append(ms_n)
    med = lambda x: float(np.median(x))  # noqa: E731
    say(f"  {'build (prep, scan, host wait + allocation, scatter)':58s} {med(t_build):9.2f} ms")
    say(f"  {'query (distance, triangle, closest point)':58s} {med(t_query):9.2f} ms   {nq / med(t_query) / 1e3:.1f} M queries / s")
    say(f"  {'sample plan + emit (points, normals)':58s} {med(t_sample):9.2f} ms")
    say(f"  {'mf_cloud_nn_dev against the vertices (build + query)':58s} {med(t_nn):9.2f} ms")
    say(f"medians of {a.reps} calls after one warm-up, between HIP events on the calls' stream")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
