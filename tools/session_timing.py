"""Times saving and loading a session at configs[4] size: one dense background map (synth.dense_room_map in a stress.make_context context, as
stress.lead_in uploads it), no objects.

  save         MaskFusion.saveSession into --dir (wall seconds; GB/s over the bytes of the file)
  load         MaskFusion.loadSession of that file (wall seconds: mf_create with its allocations, the uploads, the digests, the run table)
  pack         k_session_pack over the whole map, chunk by chunk into the staging block, without the copies (HIP events, mf_k_session_timing);
               GB/s over 48 B read + 48 B written per surfel
  digest       k_state_digest over the same surfels (HIP events); GB/s over 48 B read per surfel; and stateDigest() as a whole (wall)
  downloadMap  Model.downloadMap() of the same map (wall): three whole-buffer copies into pageable vectors and a host interleave

--dir should be a memory file system (the default is one where it exists): the question is what the library costs, not what a disk does.

    python tools/session_timing.py [--surfels 26.9e6] [--dir /dev/shm] [--reps 3]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--surfels", type=float, default=26.9e6)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1, help="1 / scale of configs[4]'s resolution (rehearsals)")
    a = ap.parse_args(argv)
    from maskfusion_amd import MaskFusion, stress, synth
    st = stress.stream(scale=a.scale)
    mf = stress.make_context(n_objects=0, scale=a.scale)
    rgb, depth, mask = st.frame(0)
    mf.processFrame(rgb, depth, mask=mask, classIDs=[0], timestamp=0)
    room = synth.dense_room_map(st.scene, int(a.surfels), last_time=1.0, furniture_above=st.masked_objects)
    mf.getBackgroundModel().uploadMap(room)
    n = mf.getBackgroundModel().lastCount()
    del room
    res = dict(surfels=n, map_bytes=n * 48)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        path = os.path.join(d, "timing.mfs")
        t = []
        for _ in range(a.reps + 1):          # (the first call allocates the staging blocks)
            t0 = time.perf_counter()
            mf.saveSession(path)
            t.append(time.perf_counter() - t0)
        size = os.path.getsize(path)
        res.update(file_bytes=size, save_s=float(np.median(t[1:])), save_first_s=t[0], save_gbps=size / float(np.median(t[1:])) / 1e9)
        ms, cnt = (C.c_float * 2)(), C.c_uint32(0)
        pk, dg = [], []
        for _ in range(a.reps + 1):
            mf._chk(mf._L.mf_k_session_timing(mf._h, 0, ms, C.byref(cnt)))
            pk.append(ms[0])
            dg.append(ms[1])
        res.update(pack_ms=float(np.median(pk[1:])), pack_gbps=96.0 * n / max(float(np.median(pk[1:])), 1e-9) / 1e6,
                   digest_ms=float(np.median(dg[1:])), digest_gbps=48.0 * n / max(float(np.median(dg[1:])), 1e-9) / 1e6)
        t0 = time.perf_counter()
        mf.stateDigest()
        res["state_digest_s"] = time.perf_counter() - t0
        t = []
        for _ in range(max(1, a.reps - 1)):
            t0 = time.perf_counter()
            m = mf.getBackgroundModel().downloadMap()
            t.append(time.perf_counter() - t0)
            del m
        res.update(download_map_s=float(np.median(t)), download_map_gbps=48.0 * n / float(np.median(t)) / 1e9)
        mf.close()
        t0 = time.perf_counter()
        mf2 = MaskFusion.loadSession(path)
        res["load_s"] = time.perf_counter() - t0
        assert mf2.getBackgroundModel().lastCount() == n
        mf2.close()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
