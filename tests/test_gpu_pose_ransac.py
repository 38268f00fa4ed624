"""The hypothesis search on the device (mf_pose_ransac_dev, maskfusion_amd.eval.ransac_correspondences(device=True) and
register_global(ransac="device")) against the numpy restatement of tests/ransac_restatement.py: statuses, counts, winner and mask exactly, the
winner's pose bit for bit.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build.

Planted cases.  max(3, ceil(0.4 m)) of the m correspondences follow gs.motion() with 1 mm of noise, the others are uniform in a 2 m cube;
the triples are default_rng's.  edge_tolerance is 0.5, so that a fair share of the triples with an outlier passes the edge test too and is
fitted and scored: with 0.1 nearly every tested triple would be a planted one.  A case's seed is the first, counted up from 1000 m, whose FIRST
triple is planted, tested and reaches 0.35 m inliers on its own: so the planted motion wins for every prefix of the triples, h = 1 included
(with one triple the share of tested triples is 0 or 1: the 5 % .. 95 % window is asserted for h >= 255).  All of this is decided on the
restatement alone, before the kernel runs."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_scene as gs  # noqa: E402
import ransac_restatement as rs  # noqa: E402
import register_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS, TILE, CHUNK = 256, 128, 2048          # the kernel's workgroup (hypotheses), LDS tile and blockIdx.y chunk (correspondences)
DIST, TOL = 0.01, 0.5
HS = (1, 255, 256, 257, 4099)                  # around the workgroup of 256 hypotheses; 4099: 17 workgroups
MS = (3, 4, 63, 64, 65, 257, 1000, TILE - 1, TILE, TILE + 1, THREADS - 1, THREADS, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)   # the last: 3 chunks
SENTINEL = 0xA5


def test_the_sizes_above_are_the_kernels(hip):
    src = open(os.path.join(ROOT, "maskfusion_amd", "csrc", "mf_register.hip")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr int (kRansacThreads|kRansacTile|kRansacChunk) = (\d+);", src)}
    assert got == {"kRansacThreads": THREADS, "kRansacTile": TILE, "kRansacChunk": CHUNK}


def _call(src, dst, tri, dist=DIST, tol=TOL, stride=3, mask=True, pose=True, m=None, h=None, null=()):
    """mf_pose_ransac_dev on (m, stride) float32 records and (h, 3) int32 triples; every output starts as SENTINEL bytes.  Returns (rc, dict)"""
    import torch
    from maskfusion_amd.lib import load, torch_device
    L = load()
    dev = torch_device()
    src, dst = np.ascontiguousarray(src, np.float32).reshape(-1, stride), np.ascontiguousarray(dst, np.float32).reshape(-1, stride)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    m = len(src) if m is None else m
    h = len(tri) if h is None else h
    up = lambda a: torch.from_numpy(a if a.size else np.zeros(4, a.dtype)).to(dev)           # noqa: E731
    fill = lambda n, dt: torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device=dev).repeat_interleave(dt).contiguous()   # noqa: E731
    d = {"src": up(src), "dst": up(dst), "tri": up(tri), "counts": fill(len(tri), 4), "status": fill(len(tri), 1), "best": fill(2, 4),
         "inlier": fill(len(src), 1), "pose": fill(12, 8)}
    p = {k: (None if k in null else v.data_ptr()) for k, v in d.items()}
    rc = L.mf_pose_ransac_dev(p["src"], p["dst"], stride, m, p["tri"], h, dist, tol, p["counts"], p["status"], p["best"],
                              p["inlier"] if mask else None, p["pose"] if pose else None, None)
    out = {k: d[k].cpu().numpy() for k in ("counts", "status", "best", "inlier", "pose")}     # (the copies wait for the null stream)
    out["counts"] = out["counts"].view(np.uint32)[:len(tri)]
    out["status"] = out["status"][:len(tri)]
    out["best"] = out["best"].view(np.int32)
    out["inlier"] = out["inlier"][:len(src)]
    return rc, out


def _untouched(out):
    return all((out[k].view(np.uint8) == SENTINEL).all() for k in ("counts", "status", "best", "inlier", "pose"))


def _agree(out, want, mask=True, pose=True):
    assert np.array_equal(out["status"], want["status"])
    assert np.array_equal(out["counts"], want["counts"])
    assert out["best"].tolist() == want["best"].tolist()
    if mask:
        assert np.array_equal(out["inlier"], want["inlier"])
    else:
        assert (out["inlier"] == SENTINEL).all()
    if pose and want["pose"] is not None:
        assert out["pose"].tobytes() == want["pose"].tobytes()
    else:
        assert (out["pose"] == SENTINEL).all()


def _planted(m):
    """(src, dst float32 (m, 3), the planted rows, triples (max(HS), 3), the seed): see the module's docstring"""
    T = gs.motion()
    n_in = max(3, math.ceil(0.4 * m))
    for seed in range(1000 * m, 1000 * m + 5000):
        rng = np.random.default_rng(seed)
        src = rng.uniform(-1, 1, (m, 3))
        dst = rng.uniform(-1, 1, (m, 3))
        planted = np.sort(rng.permutation(m)[:n_in])
        dst[planted] = src[planted] @ T[:3, :3].T + T[:3, 3] + rng.normal(scale=1e-3, size=(n_in, 3))
        tri = rng.integers(0, m, (max(HS), 3))
        if not np.isin(tri[0], planted).all():
            continue
        src, dst = src.astype(np.float32), dst.astype(np.float32)
        first = rs.search(src, dst, tri[:1], DIST, TOL)
        if first["status"][0] == 0 and first["counts"][0] >= 0.35 * m:
            return src, dst, planted, tri, seed
    raise AssertionError("no seed makes the case bite")


# ---------------- 1. planted motion ----------------
@pytest.mark.parametrize("m", MS)
def test_planted_motion_matches_the_restatement(hip, m):
    src, dst, planted, tri, seed = _planted(m)
    full = rs.search(src, dst, tri, DIST, TOL)
    share = (full["status"] == 0).mean()
    print("m %d seed %d: tested %.1f %% of %d, statuses %s, winner %s" % (m, seed, 100 * share, len(tri), np.bincount(full["status"], minlength=4).tolist(),
                                                                          full["best"].tolist()))
    for h in HS:
        want = rs.pick(full, src, dst, DIST, h)
        # the restatement alone: the case bites
        j, cnt = want["best"]
        assert j >= 0 and np.isin(tri[j], planted).all() and cnt >= 0.35 * m
        dt, dr = rr.pose_error(np.vstack([want["pose"].reshape(3, 4), [0, 0, 0, 1]]), gs.motion())
        assert dt < 0.05 and dr < 0.05                                   # the winner is the planted motion
        if h >= 255:
            assert 0.05 <= (want["status"] == 0).mean() <= 0.95
        rc, out = _call(src, dst, tri[:h])
        assert rc == 0
        _agree(out, want)
    # the optional outputs left out: the rest is the same
    want = rs.pick(full, src, dst, DIST, 257)
    for mask, pose in ((False, True), (True, False), (False, False)):
        rc, out = _call(src, dst, tri[:257], mask=mask, pose=pose)
        assert rc == 0
        _agree(out, want, mask, pose)


# ---------------- 2. edge cases ----------------
def _small():
    """40 correspondences under an exact motion (a quarter turn and an integer shift of integer points: no rounding anywhere)"""
    rng = np.random.default_rng(7)
    src = rng.permutation(np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3))[:40].astype(np.float32)
    dst = np.stack([-src[:, 1], src[:, 0], src[:, 2]], 1) + np.array([5, -3, 2], np.float32)
    return src, dst


def _noncollinear(src, rng, n):
    out = []
    while len(out) < n:
        t = rng.choice(len(src), 3, replace=False)
        if np.linalg.norm(np.cross(src[t[1]] - src[t[0]], src[t[2]] - src[t[0]])) > 0:
            out.append(t)
    return np.array(out)


def test_statuses_of_bad_triples(hip):
    src, dst = _small()
    src, dst = src.copy(), dst.copy()
    m = len(src)
    # rows 30..32: collinear in src and dst with equal spacing (passes the edge test); 33 = a copy of 34 (a zero-length edge);
    # 35: NaN in src, 36: inf in dst
    for k, x in zip((30, 31, 32), (10.0, 11.0, 12.0)):
        src[k] = [x, 0, 0]
        dst[k] = [0, x, 0]
    src[33], dst[33] = src[34], dst[34]
    src[35, 1] = np.nan
    dst[36, 2] = np.inf
    rng = np.random.default_rng(8)
    good = _noncollinear(src[:30], rng, 6)
    tri = np.array([[2, 2, 5], [5, 2, 2], [2, 5, 2], [-1, 0, 1], [0, m, 1], [0, 1, -2 ** 31], [30, 31, 32], [33, 34, 0], [0, 33, 34], [35, 0, 1], [0, 1, 36],
                    [-1, 35, 35], *good, [0, 1, 35]])
    want = rs.search(src, dst, tri, DIST, 0.1)
    assert want["status"].tolist() == [1, 1, 1, 1, 1, 1, 3, 2, 2, 3, 3, 1, 0, 0, 0, 0, 0, 0, 3]
    assert (want["counts"][want["status"] != 0] == 0).all() and (want["counts"][12:18] == 35).all()      # rows 35 and 36 (NaN, inf), 30..32 are off
    assert want["best"].tolist() == [12, 35] and not want["inlier"][[35, 36]].any()                      # ties: the smallest index
    rc, out = _call(src, dst, tri, tol=0.1)
    assert rc == 0
    _agree(out, want)
    rc2, again = _call(src, dst, tri, tol=0.1)
    assert rc2 == 0 and all(out[k].tobytes() == again[k].tobytes() for k in out)                          # two calls: the same bytes


def test_a_nan_among_the_scored_correspondences_and_strides(hip):
    src, dst = _small()
    rng = np.random.default_rng(9)
    tri = _noncollinear(src[:20], rng, 300)
    src, dst = src.copy(), dst.copy()
    src[25, 0] = np.nan
    dst[26, 1] = np.nan
    dst[27] += np.float32(0.5)                                          # an outlier
    want = rs.search(src, dst, tri, DIST, 0.1)
    assert (want["status"] == 0).all() and (want["counts"] == 37).all() and want["best"].tolist() == [0, 37]
    assert want["inlier"].sum() == 37 and not want["inlier"][[25, 26, 27]].any()
    for stride in (3, 4, 12):
        a = rng.normal(size=(len(src), stride)).astype(np.float32)
        b = rng.normal(size=(len(src), stride)).astype(np.float32)
        if stride > 3:
            a[::3, 3:], b[1::3, 3:] = np.nan, np.inf                   # what lies between the points is not read
        a[:, :3], b[:, :3] = src, dst
        rc, out = _call(a, b, tri, tol=0.1, stride=stride)
        assert rc == 0, stride
        _agree(out, want)


def test_identical_best_triples_go_to_the_smaller_index(hip):
    src, dst, planted, tri, _ = _planted(65)
    tri = tri[:300].copy()
    j = int(rs.search(src, dst, tri, DIST, TOL)["best"][0])
    tri[[120, 280]] = tri[j]                                            # two more copies of the winner ...
    tri[j] = [0, 0, 0]                                                  # ... and the first one gone
    want = rs.search(src, dst, tri, DIST, TOL)
    top = np.flatnonzero(want["counts"] == want["counts"].max())
    assert want["counts"][120] == want["counts"][280] == want["counts"].max() and len(top) >= 2 and want["best"][0] == top[0] <= 120
    rc, out = _call(src, dst, tri)
    assert rc == 0
    _agree(out, want)


def test_no_testable_triple(hip):
    src, dst = _small()
    tri = np.array([[0, 0, 1], [1, 2, 2], [40, 0, 1]])
    for s, d, t in ((src, dst, tri), (src, 2 * dst, _noncollinear(src, np.random.default_rng(10), 50)),      # the edge test drops all
                    (src[:2], dst[:2], np.array([[0, 1, 1], [0, 1, 2]])), (src[:1], dst[:1], tri), (src, dst, np.zeros((0, 3), int))):
        want = rs.search(s, d, t, DIST, 0.1)
        assert want["best"].tolist() == [-1, 0] and want["pose"] is None and not want["inlier"].any() and not want["counts"].any()
        rc, out = _call(s, d, t, tol=0.1)
        assert rc == 0
        _agree(out, want)                                               # ... which includes: d_pose keeps its SENTINEL bytes
    # m == 0, and h == 0 with every pointer of the empty side null
    rc, out = _call(np.zeros((0, 3)), np.zeros((0, 3)), tri, null=("src", "dst"))
    assert rc == 0 and out["best"].tolist() == [-1, 0] and out["status"].tolist() == [1, 1, 1] and not out["counts"].any()
    rc, out = _call(src, dst, np.zeros((0, 3), int), null=("tri", "counts", "status"))
    assert rc == 0 and out["best"].tolist() == [-1, 0] and not out["inlier"].any() and (out["pose"] == SENTINEL).all()


def test_edge_tolerance_zero_passes_a_congruent_triple(hip):
    src, dst = _small()
    tri = _noncollinear(src, np.random.default_rng(11), 200)
    want = rs.search(src, dst, tri, DIST, 0.0)
    assert (want["status"] == 0).all() and (want["counts"] == 40).all()
    rc, out = _call(src, dst, tri, tol=0.0)
    assert rc == 0
    _agree(out, want)
    # the smallest stretch of one point: its triples fail at tolerance 0 and pass at 0.1
    d2 = dst.copy()
    d2[tri[0, 0]] += np.float32(0.25)
    w0, w1 = rs.search(src, d2, tri, DIST, 0.0), rs.search(src, d2, tri, DIST, 0.1)
    assert w0["status"][0] == 2 and (w0["status"] == 2).sum() < len(tri) and (w1["status"] == 0).sum() > (w0["status"] == 0).sum()
    for tol, w in ((0.0, w0), (0.1, w1)):
        rc, out = _call(src, d2, tri, tol=tol)
        assert rc == 0
        _agree(out, w)


# ---------------- 3. argument checks ----------------
def test_argument_errors_write_nothing(hip):
    src, dst = _small()
    tri = _noncollinear(src, np.random.default_rng(12), 20)
    rc, out = _call(src, dst, tri)
    assert rc == 0 and not _untouched(out)
    big = (1 << 24) + 1
    for kw in ({"null": ("src",)}, {"null": ("dst",)}, {"null": ("tri",)}, {"null": ("counts",)}, {"null": ("status",)}, {"null": ("best",)},
               {"m": -1}, {"h": -1}, {"m": big}, {"h": big}, {"dist": 0.0}, {"dist": -1.0}, {"dist": float("nan")}, {"dist": float("inf")},
               {"tol": -0.01}, {"tol": 1.0}, {"tol": float("nan")}, {"tol": float("inf")}):
        rc, out = _call(src, dst, tri, **kw)
        assert rc == -1 and _untouched(out), kw
    import torch
    from maskfusion_amd.lib import load, torch_device
    t = torch.zeros(64, dtype=torch.int32, device=torch_device())       # every pointer: 256 bytes that stay zero
    for stride in (2, 0, -3):
        assert load().mf_pose_ransac_dev(t.data_ptr(), t.data_ptr(), stride, 4, t.data_ptr(), 1, 0.1, 0.1, t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                         None, None, None) == -1
        assert not t.cpu().numpy().any()


# ---------------- 4. end to end ----------------
def test_python_search_returns_the_documented_dictionary(hip):
    from maskfusion_amd import eval as ev
    src, dst, planted, tri, seed = _planted(257)
    res = ev.ransac_correspondences(src, dst, DIST, hypotheses=2000, seed=3, edge_tolerance=TOL, device=True)
    t3 = np.random.default_rng(3).integers(0, 257, (2000, 3))
    want = rs.search(src, dst, t3, DIST, TOL)
    assert set(res) == {"T", "inliers", "inlier_mask", "hypotheses", "tested"}
    assert res["hypotheses"] == 2000 and res["tested"] == int((want["status"] == 0).sum()) and res["inliers"] == want["best"][1]
    assert res["inlier_mask"].dtype == bool and np.array_equal(res["inlier_mask"], want["inlier"].astype(bool))
    mask = res["inlier_mask"]
    assert np.array_equal(res["T"], ev.align_horn(src[mask].astype(np.float64), dst[mask].astype(np.float64)))
    dt, dr = rr.pose_error(res["T"], gs.motion())
    assert dt < 5e-3 and dr < 5e-3                                      # 1 mm of noise on a hundred inliers
    assert ev.ransac_correspondences(src[:2], dst[:2], DIST, device=True)["T"] is None


def test_register_global_on_the_device_search(hip):
    """the gates tests/test_gpu_fpfh.py states for the host search"""
    from maskfusion_amd import eval as ev
    est, en, ref, rn, T = gs.exact_pair()
    res = ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=0, ransac="device")
    dt, dr = rr.pose_error(res["T"], T)
    ct, cr = rr.pose_error(res["coarse"]["T"], T)
    print("coarse:", {k: v for k, v in res["coarse"].items() if k != "T"}, "error %.3g m %.3g deg" % (ct, np.degrees(cr)), "final", dt, dr)
    assert ct <= 1.5 * gs.VOXEL and np.degrees(cr) <= 5.0
    assert res["converged"] and dt < 1e-5 and dr < 1e-5
    again = ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=0, refine=False, ransac="device")
    assert again["reason"] == "not refined" and again["coarse"]["inliers"] == res["coarse"]["inliers"]
    assert np.array_equal(again["T"], res["coarse"]["T"])
    with pytest.raises(ValueError):
        ev.register_global(est, ref, gs.VOXEL, ransac="gpu")
