"""Times the run evaluation's nearest-neighbour kernels (mf_cloud_nn_dev, mf_model_cloud_nn_dev; maskfusion_amd/csrc/mf_eval.hip) at configs[4]
size: a dense room map of 26.9 M points (synth.dense_room_map, the background of stress.make_context's scenario) as the targets, 5 M queries
sampled from it and jittered by N(0, 5 mm) per axis, radius 5 cm.

  grid build   mf_cloud_nn_dev with no queries (count, scan, scatter)
  query        the same call with the queries, minus the build
  live model   mf_model_cloud_nn_dev against the same map uploaded into a stress.make_context context (gather + build + query)
  icp step     mf_cloud_icp_step_dev (point-to-plane, the map's own normals) on the same clouds next to the mf_cloud_nn_dev query, both as
               medians of 20 calls after 5 warm-ups, and their ratio; then the wall time of a whole eval.register() from a start 1 degree
               and 1 cm off
  normals      mf_cloud_normals_dev on the targets (grid build + walk and moments + eigen-solve), radius 2 x --radius as the evaluation
               command's --estimate-normals takes it, as the median of 5 calls after 1 warm-up; minus the grid build at that radius
  global       mf_cloud_fpfh_dev on --keys points of the map with the map's normals at --fpfh-radius, and mf_feature_match_dev of those
               descriptors against the descriptors of as many other points of the map (33 values each): the two device calls of
               eval.register_global at 50 k x 50 k key points, each as the median of 5 calls after 1 warm-up
  ransac       mf_pose_ransac_dev on --triples triples x --correspondences correspondences (40 % under one rigid motion with 1 mm of noise, the
               others uniform in a 2 m cube; inlier distance 1 cm, edge tolerance 0.1): the median of 5 calls after 1 warm-up, next to the wall
               time of eval.ransac_correspondences on the host (numpy) for the same input and seed; --ransac-only runs this line alone

Device times are medians of 10 calls after 2 warm-up calls, between HIP events on the call's stream.  One CPU line for contrast:
scipy.spatial.cKDTree with 16 workers on the same clouds (tree build + query), if scipy is present.

    python tools/eval_timing.py [--targets 26.9e6] [--queries 5e6] [--radius 0.05] [--no-cpu] [--no-live] [--no-icp] [--no-normals]
                                [--no-global] [--keys 50000] [--fpfh-radius 0.25] [--no-ransac] [--ransac-only] [--triples 20000]
                                [--correspondences 50000]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, stream, reps=10, warm=2):
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


def _ransac_line(a, L):
    import torch
    from maskfusion_amd import eval as ev
    from maskfusion_amd import synth
    m, h = int(a.correspondences), int(a.triples)
    rng = np.random.default_rng(0)
    T = synth.make_pose(synth.rot_xyz(*np.deg2rad([40.0, -70.0, 110.0])), [2.0, -1.0, 2.0])
    src = rng.uniform(-1, 1, (m, 3))
    dst = rng.uniform(-1, 1, (m, 3))
    planted = rng.permutation(m)[:int(0.4 * m)]
    dst[planted] = src[planted] @ T[:3, :3].T + T[:3, 3] + rng.normal(scale=1e-3, size=(len(planted), 3))
    src, dst = src.astype(np.float32), dst.astype(np.float32)
    tri = np.random.default_rng(0).integers(0, m, (h, 3)).astype(np.int32)          # the draw of ransac_correspondences(seed=0)
    s = torch.cuda.current_stream()
    ds, dd, dtri = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), torch.from_numpy(tri).cuda()
    counts = torch.empty(h, dtype=torch.int32, device="cuda")
    status = torch.empty(h, dtype=torch.uint8, device="cuda")
    best = torch.empty(2, dtype=torch.int32, device="cuda")
    mask = torch.empty(m, dtype=torch.uint8, device="cuda")
    pose = torch.empty(12, dtype=torch.float64, device="cuda")

    def call():
        rc = L.mf_pose_ransac_dev(ds.data_ptr(), dd.data_ptr(), 3, m, dtri.data_ptr(), h, 0.01, 0.1, counts.data_ptr(), status.data_ptr(), best.data_ptr(),
                                  mask.data_ptr(), pose.data_ptr(), s.cuda_stream)
        assert rc == 0, rc
    td = _median_ms(call, s, reps=5, warm=1)
    tested = int((status == 0).sum().item())
    t0 = time.perf_counter()
    dev = ev.ransac_correspondences(src, dst, 0.01, hypotheses=h, seed=0, device=True)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = ev.ransac_correspondences(src, dst, 0.01, hypotheses=h, seed=0)
    t_host = time.perf_counter() - t0
    print(f"ransac     : median {td[0]:.2f} ms (min {td[1]:.2f}, max {td[2]:.2f}) for {h} triples x {m} correspondences, {tested} tested: "
          f"{tested * m / td[0] / 1e6:.1f} G scores/s; winner {best.cpu().tolist()}; eval.ransac_correspondences device {1e3 * t_dev:.0f} ms wall "
          f"({dev['inliers']} inliers), host {1e3 * t_host:.0f} ms wall ({host['inliers']} inliers, {host['tested']} tested)")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=float, default=26.9e6)
    ap.add_argument("--queries", type=float, default=5e6)
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-live", action="store_true")
    ap.add_argument("--no-icp", action="store_true")
    ap.add_argument("--no-normals", action="store_true")
    ap.add_argument("--no-global", action="store_true")
    ap.add_argument("--keys", type=float, default=50e3)
    ap.add_argument("--fpfh-radius", type=float, default=0.25)
    ap.add_argument("--no-ransac", action="store_true")
    ap.add_argument("--ransac-only", action="store_true")
    ap.add_argument("--triples", type=float, default=20e3)
    ap.add_argument("--correspondences", type=float, default=50e3)
    a = ap.parse_args(argv)
    import torch
    from maskfusion_amd import stress, synth
    from maskfusion_amd.lib import load
    L = load()
    if a.ransac_only:
        _ransac_line(a, L)
        return 0
    t0 = time.perf_counter()
    st = stress.stream()
    room = synth.dense_room_map(st.scene, int(a.targets), last_time=1.0, furniture_above=st.masked_objects)
    rng = np.random.default_rng(0)
    nq = int(a.queries)
    xyz = np.ascontiguousarray(room[:, :3])
    q = (xyz[rng.integers(0, len(xyz), nq)] + rng.normal(scale=0.005, size=(nq, 3))).astype(np.float32)
    print(f"clouds: {len(xyz)} targets, {nq} queries, radius {a.radius} m (generated in {time.perf_counter() - t0:.1f} s)")
    dt, dq = torch.from_numpy(xyz).cuda(), torch.from_numpy(q).cuda()
    need = C.c_uint64(0)
    assert L.mf_cloud_nn_workspace(len(xyz), C.byref(need)) == 0
    ws = torch.empty(int(need.value), dtype=torch.uint8, device="cuda")
    dist = torch.empty(nq, dtype=torch.float32, device="cuda")
    idx = torch.empty(nq, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()

    def call(n_query):
        rc = L.mf_cloud_nn_dev(dt.data_ptr(), 3, len(xyz), dq.data_ptr(), 3, n_query, None, a.radius, dist.data_ptr(), idx.data_ptr(),
                               ws.data_ptr(), int(need.value), s.cuda_stream)
        assert rc == 0, rc
    build = _median_ms(lambda: call(0), s)
    full = _median_ms(lambda: call(nq), s)
    hits = (idx >= 0).float().mean().item()
    N, B = len(xyz), 64
    while B < 2 * N:
        B <<= 1
    # algorithmic bytes: build = targets read twice (count, scatter) + rank written / read + records written + bucket array memset, counted,
    # scanned (read twice, written once); query = queries read + outputs written + the grid's start pairs (the bucket scans hit cached lines)
    b_build = N * 12 * 2 + N * 4 * 2 + N * 16 + (B + 1) * 4 * 4
    print(f"workspace: {need.value / 2**20:.0f} MiB ({B} buckets)")
    print(f"grid build : median {build[0]:.2f} ms (min {build[1]:.2f}, max {build[2]:.2f}); algorithmic bytes {b_build / 1e9:.2f} GB "
          f"-> {b_build / build[0] / 1e6:.0f} GB/s")
    qm = full[0] - build[0]
    print(f"query      : median {qm:.2f} ms (build + query {full[0]:.2f} ms, min {full[1]:.2f}, max {full[2]:.2f}); "
          f"{nq / qm / 1e3:.0f} M queries/s; hits {hits:.4f}")
    print(f"build + query on {N / 1e6:.1f} M targets x {nq / 1e6:.1f} M queries: {full[0]:.2f} ms (target < 1000 ms)")
    if not a.no_icp:
        from maskfusion_amd import eval as ev
        drec = torch.from_numpy(room).cuda()                # 12-float records: the normal at offset 8
        t0 = time.perf_counter()
        reg = ev.Registration(drec, a.radius, 8, nq)
        torch.cuda.synchronize()
        t_build = time.perf_counter() - t0
        out29 = torch.zeros(29, dtype=torch.float64, device="cuda")

        def step():
            rc = L.mf_cloud_icp_step_dev(reg._ws.data_ptr(), reg._need, dq.data_ptr(), 3, nq, None, out29.data_ptr(), s.cuda_stream)
            assert rc == 0, rc
        full20 = _median_ms(lambda: call(nq), s, reps=20, warm=5)
        build20 = _median_ms(lambda: call(0), s, reps=20, warm=5)
        step20 = _median_ms(step, s, reps=20, warm=5)
        q20 = full20[0] - build20[0]
        pairs = int(out29[28].item())
        print(f"icp step   : median {step20[0]:.2f} ms (min {step20[1]:.2f}, max {step20[2]:.2f}) against the nn query's {q20:.2f} ms "
              f"(build + query {full20[0]:.2f} - build {build20[0]:.2f}; 20 calls after 5 warm-ups): ratio {step20[0] / q20:.3f}; "
              f"{pairs} pairs (nn hits {int((idx >= 0).sum().item())}); workspace {reg._need / 2**20:.0f} MiB, its build {1e3 * t_build:.0f} ms wall")
        T0 = synth.make_pose(synth.rot_xyz(*np.deg2rad([1.0, -1.0, 1.0])), [0.01, -0.01, 0.01])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ev.register(dq, drec, a.radius, T0=T0, ref_normals=8, schedule=[2 * a.radius, a.radius])
        t_reg = time.perf_counter() - t0
        print(f"register   : {t_reg:.2f} s wall for {res['iterations']} iterations at radii {2 * a.radius:g}, {a.radius:g} (converged {res['converged']}, "
              f"inlier share {res['inlier_share']:.4f}, rmse {res['rmse']:.3g} m, |t| {np.linalg.norm(res['T'][:3, 3]):.2e} m, "
              f"angle {ev.rotation_angle(res['T'][:3, :3]):.2e} rad from the identity)")
        del drec, reg
    if not a.no_normals:
        N, rn = len(xyz), 2 * a.radius
        need_n = C.c_uint64(0)
        assert L.mf_cloud_normals_workspace(N, C.byref(need_n)) == 0
        ws_n = torch.empty(int(need_n.value), dtype=torch.uint8, device="cuda")
        nrm4 = torch.empty((N, 4), dtype=torch.float32, device="cuda")
        cnt = torch.empty(N, dtype=torch.int32, device="cuda")

        def normals():
            rc = L.mf_cloud_normals_dev(dt.data_ptr(), 3, N, rn, 5, None, nrm4.data_ptr(), cnt.data_ptr(), ws_n.data_ptr(), int(need_n.value),
                                        s.cuda_stream)
            assert rc == 0, rc

        def build_n():
            rc = L.mf_cloud_nn_dev(dt.data_ptr(), 3, N, dq.data_ptr(), 3, 0, None, rn, dist.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                                   int(need.value), s.cuda_stream)
            assert rc == 0, rc
        tn = _median_ms(normals, s, reps=5, warm=1)
        tb = _median_ms(build_n, s, reps=5, warm=1)
        k_mean = cnt.double().mean().item()
        print(f"normals    : median {tn[0]:.2f} ms (min {tn[1]:.2f}, max {tn[2]:.2f}) for {N / 1e6:.1f} M points at radius {rn:g} m, {k_mean:.1f} "
              f"neighbours a point; walk + solve {tn[0] - tb[0]:.2f} ms (grid build {tb[0]:.2f} ms): {N * k_mean / (tn[0] - tb[0]) / 1e6:.1f} G neighbours/s; "
              f"{int(torch.isnan(nrm4[:, 3]).sum().item())} points without a normal; workspace {need_n.value / 2**20:.0f} MiB")
        del ws_n, nrm4, cnt
    if not a.no_global:
        nk = int(min(a.keys, len(room) // 2))
        pick = rng.choice(len(room), 2 * nk, replace=False)
        need_f = C.c_uint64(0)
        assert L.mf_cloud_fpfh_workspace(nk, C.byref(need_f)) == 0
        ws_f = torch.empty(int(need_f.value), dtype=torch.uint8, device="cuda")
        desc, cnts = [], None
        for half in (pick[:nk], pick[nk:]):
            rec = torch.from_numpy(np.ascontiguousarray(room[half][:, [0, 1, 2, 8, 9, 10]])).cuda()
            out = torch.empty((nk, 33), dtype=torch.float32, device="cuda")
            cnts = torch.empty((nk, 34), dtype=torch.int32, device="cuda")

            def fpfh_call():
                rc = L.mf_cloud_fpfh_dev(rec.data_ptr(), 6, 3, nk, a.fpfh_radius, out.data_ptr(), cnts.data_ptr(), ws_f.data_ptr(), int(need_f.value),
                                         s.cuda_stream)
                assert rc == 0, rc
            tf = _median_ms(fpfh_call, s, reps=5, warm=1)
            desc.append(out)
        midx = torch.empty(nk, dtype=torch.int32, device="cuda")
        md2 = torch.empty(nk, dtype=torch.float32, device="cuda")

        def match_call():
            rc = L.mf_feature_match_dev(desc[0].data_ptr(), nk, desc[1].data_ptr(), nk, 33, midx.data_ptr(), md2.data_ptr(), s.cuda_stream)
            assert rc == 0, rc
        tm = _median_ms(match_call, s, reps=5, warm=1)
        print(f"fpfh       : median {tf[0]:.2f} ms (min {tf[1]:.2f}, max {tf[2]:.2f}) for {nk} points at radius {a.fpfh_radius:g} m, "
              f"{cnts[:, 33].double().mean().item():.1f} counted pairs a point; {int(torch.isnan(desc[1][:, 0]).sum().item())} rows without a descriptor; "
              f"workspace {need_f.value / 2**20:.1f} MiB")
        print(f"match      : median {tm[0]:.2f} ms (min {tm[1]:.2f}, max {tm[2]:.2f}) for {nk} x {nk} descriptors of 33 values: "
              f"{nk * nk * 33 / tm[0] / 1e6:.1f} G terms/s; {int((midx >= 0).sum().item())} queries matched")
        del ws_f, desc, cnts
    if not a.no_ransac:
        _ransac_line(a, L)
    if not a.no_live:
        mf = stress.make_context()
        rgb, depth, mask = st.frame(0)
        mf.processFrame(rgb, depth, mask=mask, timestamp=0)
        mf.getBackgroundModel().uploadMap(room)
        mf.sync()
        live = _median_ms(lambda: mf.modelCloudNN(0, dq, a.radius), s)
        d2, i2 = mf.modelCloudNN(0, dq, a.radius)
        same = bool(torch.equal(d2, dist)) and bool(torch.equal(i2, idx))
        print(f"live model : median {live[0]:.2f} ms (min {live[1]:.2f}, max {live[2]:.2f}) for {mf.getBackgroundModel().lastCount()} surfels "
              f"(gather + build + query + host waits); same result as the plain call: {same}")
        mf.close()
    if not a.no_cpu:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            print("cpu        : scipy not present, skipped")
            return 0
        t0 = time.perf_counter()
        tree = cKDTree(xyz)
        t1 = time.perf_counter()
        kd, _ = tree.query(q, k=1, distance_upper_bound=a.radius, workers=16)
        t2 = time.perf_counter()
        gd = dist.cpu().numpy()
        both = np.isfinite(kd) & np.isfinite(gd)
        print(f"cpu        : scipy.spatial.cKDTree (16 workers, CPU): build {1e3 * (t1 - t0):.0f} ms + query {1e3 * (t2 - t1):.0f} ms = "
              f"{1e3 * (t2 - t0):.0f} ms; max |d_gpu - d_cpu| over common hits {np.abs(gd[both] - kd[both]).max():.2e} m")
    return 0


if __name__ == "__main__":
    sys.exit(main())
