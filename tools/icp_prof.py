"""In-kernel shader-clock stamps of the single-model Gauss-Newton launches ("icpProfile": thread 0 of workgroup 0 of every k_icp_iter launch of a
VGA tracking step), averaged over frames and printed per launch and per launch form.      python tools/icp_prof.py

The eight stamps of a launch and what the seven phases between them bracket:
  0 -> 1  issue loads    the 6 x slots streamed loads of the frame's vertex / normal maps, with their address arithmetic.  Stamp 0 stands behind the
                         issue of the state's load; the scalar loads of the kernel arguments lie in front of it and are in no phase
  1 -> 2  reduce         issue of the loads of the previous launch's partials, their cold read, fp32 sums, two barriers, row sums
  2 -> 3  solve + pose   gn_finish_wg in wavefront 0 (stamps 8..11 lie inside it: system in registers, LDL^T, exp + composition, exchange)
  3 -> 4  barrier        the other wavefronts' wait ends
  4 -> 5  pixels         pose from LDS, projections, gathers of the model maps, products (ends with vmcnt(0))
  5 -> 6  block sum      block_sum29_lds
  6 -> 7  store          the partial's store has left
Launch 0 of a step has no prologue (stamp 2 = stamp 1).  Launches 0..3 are level 2 and 4..8 level 1 (both k_icp_iter<256, 1>; launch 4 reduces
level 2's 75 partials), 9..18 level 0 (<512, 3>; launch 9 reduces level 1's 300 partials, the others 240).
The last column, stamp 0 of the next launch minus stamp 0 of this one, is the launch's share of the dependent chain including everything no phase
holds (the argument loads, the dispatch).  s_memtime is not synchronised between XCDs: the column means something only where workgroup 0 of both
launches ran on the same XCD -- the level-0 launches in practice; the coarse rows show differences of millions of ticks and are not summarised."""
import sys

import numpy as np

sys.path.insert(0, ".")
import bench  # noqa: E402
from maskfusion_amd import MaskFusion  # noqa: E402

PHASES = ["issue", "reduce", "solve", "barrier", "pixels", "blocksum", "store"]


def stamps(frames):
    mf = MaskFusion(640, 480, 528, 528, 320, 240, icpThresh=100.0, so3=False, enableMultipleModels=False)
    mf.setParam("icpProfile", 1)
    acc = []
    for k in list(range(12)) + list(range(10, 0, -1)):
        mf.processFrame(frames[k][0], frames[k][1])
        if mf.getTick() > 3:
            acc.append(mf.debugRead("icp_prof").astype(np.int64))
    mf.close()
    return np.array(acc)  # frames x 19 x 16


def report(a):
    np.set_printoptions(linewidth=200, suppress=True)
    main = a[:, :, :8]
    d = np.diff(main, axis=2).mean(0)  # 19 x 7
    total = (main[:, :, 7] - main[:, :, 0]).mean(0)
    reduce_done = (main[:, :, 2] - main[:, :, 0]).mean(0)
    period = np.append(np.median(main[:, 1:, 0] - main[:, :-1, 0], axis=0), 0)
    print("ticks (s_memtime) per phase, one row per launch; cols: " + ", ".join(PHASES) + " | total | stamp 0 -> reduce done | stamp 0 -> next launch's stamp 0")
    print(np.round(np.column_stack([d, total, reduce_done, period])).astype(int))
    for name, rows in (("coarse <256, 1>, launches 1..8", slice(1, 9)), ("level 0 <512, 3>, launches 10..18", slice(10, 19))):
        print(f"{name}: " + "  ".join(f"{p} {v:.0f}" for p, v in zip(PHASES, d[rows].mean(0))) +
              f"  | total {total[rows].mean():.0f}  reduce done at {reduce_done[rows].mean():.0f}")
    print(f"level 0, launch to launch (launches 10..17): {period[10:18].mean():.0f}")
    s = a[:, 1:, :]
    seq = np.stack([s[:, :, 2], s[:, :, 8], s[:, :, 9], s[:, :, 10], s[:, :, 11], s[:, :, 3]], axis=2)
    print("inside the solve, mean over launches 1..18: unpack, LDL^T, exp + compose, exchange + state writes, return + s_pose tail")
    print(np.round(np.diff(seq, axis=2).mean((0, 1))).astype(int))


if __name__ == "__main__":
    _, frames = bench.gen_frames(bench.CONFIGS["1"], 12, 1)
    report(stamps(frames))
