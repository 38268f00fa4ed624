"""Times map merging (mf_cloud_merge_dev; maskfusion_amd/csrc/mf_merge.hip) at the map sizes of configs[4]: n_target = n_source = 3.4 M (an
object map) and 26.9 M (the background), with half of the sources having a partner.

The target is the dense room map of maskfusion_amd.synth at that many surfels.  The first half of the sources are target surfels drawn at
random and jittered by a tenth of the search radius (they find a partner); the second half are target surfels moved 50 m away (they are
appended).  The search radius is maskfusion_amd.merge.default_radius of the target, the normal gate the default.  Between HIP events on the
call's stream, the median of --reps calls after one warm-up; the call's two host waits are inside the interval.  Beside it the numpy
restatement of the tests (tests/merge_restatement.py: brute-force partner search, a Python loop for the merges) on the first --host-size
surfels of both maps, on the wall clock.  A report: nothing is gated on a time.

    python tools/merge_timing.py [--sizes 3.4e6,26.9e6] [--reps 3] [--host-size 90000] [--out profiles/merge_timing.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sources(target, radius, rng):
    n = len(target)
    half = n // 2
    on = target[rng.integers(0, n, half)].copy()
    on[:, :3] += rng.normal(scale=0.1 * radius, size=(half, 3)).astype(np.float32)
    off = target[rng.integers(0, n, n - half)].copy()
    off[:, 0] += np.float32(50.0)
    src = np.concatenate([on, off])
    return src[rng.permutation(n)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3.4e6,26.9e6")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-size", type=int, default=90000, help="surfels per map of the host restatement's run (0: skip it)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from maskfusion_amd import merge, stress, synth
    from maskfusion_amd.lib import load
    L = load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    s = torch.cuda.current_stream()
    st = stress.stream()
    for size in [int(float(x)) for x in a.sizes.split(",") if x.strip()]:
        t0 = time.perf_counter()
        target = synth.dense_room_map(st.scene, size, last_time=1.0, furniture_above=st.masked_objects)
        radius = merge.default_radius(target)
        src = sources(target, radius, np.random.default_rng(0))
        nt, ns = len(target), len(src)
        dt, ds = torch.from_numpy(target).cuda(), torch.from_numpy(src).cuda()
        out = torch.empty((nt + ns, 12), dtype=torch.float32, device="cuda")
        match = torch.empty(ns, dtype=torch.int32, device="cuda")
        need = C.c_uint64(0)
        assert L.mf_cloud_merge_workspace(nt, ns, C.byref(need)) == 0
        ws = torch.empty(int(need.value), dtype=torch.uint8, device="cuda")
        n_out, stats = C.c_int64(0), (C.c_uint64 * 4)()
        say(f"n_target = n_source = {nt}: radius {radius:.5f} m, workspace {need.value / 2 ** 20:.0f} MiB (set up in {time.perf_counter() - t0:.1f} s)")
        ms = []
        for rep in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            rc = L.mf_cloud_merge_dev(dt.data_ptr(), nt, ds.data_ptr(), ns, None, radius, float(merge.COS_HALF_RAD), out.data_ptr(), nt + ns, C.byref(n_out),
                                      match.data_ptr(), stats, ws.data_ptr(), int(need.value), s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            if rc != 0:
                raise SystemExit(f"mf_cloud_merge_dev failed with code {rc}: {L.mf_last_error(None).decode()}")
            if rep:
                ms.append(e0.elapsed_time(e1))
        st4 = [int(v) for v in stats]
        say(f"  mf_cloud_merge_dev   {float(np.median(ms)):9.2f} ms   (median of {len(ms)}; averaged {st4[0]}, confidence only {st4[1]}, appended {st4[2]}, "
            f"dropped {st4[3]}, n_out {n_out.value})")
        if a.host_size and size == int(float(a.sizes.split(",")[0])):
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import merge_restatement as mr
            h = min(a.host_size, nt)
            ht = target[:h]
            hs = sources(ht, radius, np.random.default_rng(1))
            t0 = time.perf_counter()
            rec, hm, hstats = mr.merge(ht, hs, None, radius, float(merge.COS_HALF_RAD))
            sec = time.perf_counter() - t0
            say(f"  host restatement     {sec:9.1f} s    at n_target = n_source = {h} (numpy brute force; stats {hstats})")
        del dt, ds, out, match, ws, target, src
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
