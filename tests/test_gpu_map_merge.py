"""Map-to-map fusion on the device (mf_cloud_merge_dev, maskfusion_amd.merge.merge_maps) against the numpy restatement of
tests/merge_restatement.py: every output record bit for bit, n_out, d_match and the four counts exactly.  Runs on the MI355X (-m gpu) and, with
MF_EMU=1, on the CPU-executed build.

Inputs are surfels of tests/redetect_scene.py (the 0.5 m object, about 6 000 surfels) with confidences, radii, colours and stamps of their
own; the source of a general case is given in the frame of the NEW model, so that rsn.motion() -- a 120 degree rotation and a translation --
carries it onto the target.  Every case first asserts on the RESTATEMENT alone what makes it bite, then holds the kernel to it."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_restatement as mr  # noqa: E402
import redetect_scene as rsn  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SENTINEL = 0xA5
EINVAL, ENOMEM = -1, -4
RADIUS = 0.004                     # the spacing of the full object's surfels is about 0.007: most fresh surfels find no partner
SIZES = [(0, 0), (0, 65), (65, 0), (1, 1), (1, 63), (63, 1), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255), (257, 4099), (4099, 257), (4099, 4099)]

_pool = {}


def pool():
    """the object's surfels in a fixed shuffled order, with attributes of their own; read-only"""
    if not _pool:
        rec = rsn.object_records(9000, seed=5)
        rng = np.random.default_rng(11)
        rec = rec[rng.permutation(len(rec))]
        n = len(rec)
        rec[:, 3] = rng.uniform(1.0, 20.0, n)
        rec[:, 4] = rng.integers(0, 1 << 24, n).astype(np.float32)
        rec[:, 5] = rng.integers(0, 7, n)
        rec[:, 6] = rng.integers(1, 50, n)
        rec[:, 7] = rec[:, 6] + rng.integers(0, 50, n)
        rec[:, 11] = rng.uniform(0.003, 0.0065, n)        # 0.0065 > 1.5 * 0.003: both branches of the merge occur
        rec.setflags(write=False)
        _pool["p"] = rec
    return _pool["p"]


def near(rec, rng, sigma=0.0005):
    """other surfels on the same surface: positions and normals jittered, attributes drawn anew"""
    out = np.array(rec, np.float32)
    n = len(out)
    out[:, :3] += rng.normal(scale=sigma, size=(n, 3)).astype(np.float32)
    nm = out[:, 8:11] + rng.normal(scale=0.05, size=(n, 3)).astype(np.float32)
    out[:, 8:11] = nm / np.linalg.norm(nm, axis=1, keepdims=True)
    out[:, 3] = rng.uniform(1.0, 20.0, n)
    out[:, 4] = rng.integers(0, 1 << 24, n).astype(np.float32)
    out[:, 7] = rng.integers(1, 120, n)
    out[:, 11] = rng.uniform(0.003, 0.0065, n)
    return out


def general(nt, ns):
    """(target, source in the new model's frame, T = rsn.motion()): half of the sources lie on target surfels, the others are fresh surfels of
    the object"""
    p = pool()
    assert len(p) >= 4099 + 4099
    rng = np.random.default_rng(1000 * nt + ns)
    target = p[:nt].copy()
    half = ns // 2 if nt else 0
    on = near(p[rng.integers(0, max(nt, 1), half)], rng) if half else p[:0].copy()
    src = np.concatenate([on, p[4099:4099 + ns - half]])
    src = src[rng.permutation(len(src))]
    T = rsn.motion()
    return target, rsn.moved_records(src, np.linalg.inv(T)), T


def call(target, source, T=None, radius=RADIUS, min_cos=0.0, capacity=None, want_match=True, null=(), nt=None, ns=None, ws_short=0, offset=(),
         ws_offset=0):
    """mf_cloud_merge_dev on device copies; the output and d_match start as SENTINEL bytes.  Returns (rc, dict)"""
    import torch
    from maskfusion_amd.lib import load, torch_device
    L = load()
    dev = torch_device()
    target, source = np.ascontiguousarray(target, np.float32).reshape(-1, 12), np.ascontiguousarray(source, np.float32).reshape(-1, 12)
    nt = len(target) if nt is None else nt
    ns = len(source) if ns is None else ns
    cap = len(target) + len(source) if capacity is None else capacity

    def up(a):                      # (four floats of slack in front: a record pointer can be pushed off its alignment)
        return torch.from_numpy(np.concatenate([np.zeros(16, np.float32), a.reshape(-1)])).to(dev)

    d_t, d_s = up(target), up(source)
    d_o = torch.full((16 * 4 + max(cap, 1) * 48,), SENTINEL, dtype=torch.uint8, device=dev)
    d_m = torch.full((max(len(source), 1) * 4,), SENTINEL, dtype=torch.uint8, device=dev)
    need = C.c_uint64(0)
    assert L.mf_cloud_merge_workspace(len(target), len(source), C.byref(need)) == 0 and need.value > 0 and need.value % 256 == 0
    ws = torch.zeros(int(need.value) + 256, dtype=torch.uint8, device=dev)
    ptr = {"target": d_t.data_ptr() + 64, "source": d_s.data_ptr() + 64, "out": d_o.data_ptr() + 64, "match": d_m.data_ptr() if want_match else None,
           "ws": ws.data_ptr() + ws_offset}
    for k in offset:
        ptr[k] += 4
    for k in null:
        ptr[k] = None
    n_out, stats = C.c_int64(-7), (C.c_uint64 * 4)(9, 9, 9, 9)
    T16 = None if T is None else np.ascontiguousarray(np.asarray(T, np.float32).T.reshape(16))
    rc = L.mf_cloud_merge_dev(ptr["target"], nt, ptr["source"], ns, T16.ctypes.data if T16 is not None else None, radius, min_cos, ptr["out"], cap,
                              None if "n_out" in null else C.byref(n_out), ptr["match"], None if "stats" in null else stats, ptr["ws"],
                              int(need.value) - ws_short, None)
    raw = d_o.cpu().numpy()[64:]
    out = {"n_out": n_out.value, "stats": [int(v) for v in stats], "raw": raw, "match_raw": d_m.cpu().numpy()}
    if rc == 0:
        out["records"] = raw[:n_out.value * 48].view(np.float32).reshape(-1, 12)
        out["match"] = out["match_raw"].view(np.int32)[:len(source)]
    return rc, out


def untouched(out):
    return (out["raw"] == SENTINEL).all()


def agree(out, want):
    rec, match, stats = want
    assert out["n_out"] == len(rec) and out["stats"] == stats and sum(stats) == len(match)
    assert np.array_equal(out["match"], match)
    same = mr.bits(out["records"]) == mr.bits(rec)
    assert same.all(), "records differ at rows %s" % np.flatnonzero(~same.all(1))[:8]
    assert (out["raw"][len(rec) * 48:] == SENTINEL).all()          # nothing written behind the merged map


def held(target, source, T=None, radius=RADIUS, min_cos=0.0, want=None):
    want = mr.merge(target, source, T, radius, min_cos) if want is None else want
    rc, out = call(target, source, T, radius, min_cos)
    assert rc == 0
    agree(out, want)
    return want


# ---------------- the sizes ----------------
def test_the_motion_is_a_120_degree_rotation(hip):
    R = rsn.motion()[:3, :3]
    assert abs(np.degrees(np.arccos((np.trace(R) - 1) / 2)) - 120.0) < 1e-6 and np.linalg.norm(rsn.motion()[:3, 3]) > 0.1


@pytest.mark.parametrize("nt,ns", SIZES)
def test_sizes(hip, nt, ns):
    target, source, T = general(nt, ns)
    assert (len(target), len(source)) == (nt, ns)
    want = mr.merge(target, source, T, RADIUS, float(mr_cos()))
    rec, match, stats = want
    print(nt, ns, "stats", stats)
    if nt >= 255 and ns >= 255:                                     # both branches, appended sources and lists longer than one
        assert stats[0] > 20 and stats[1] > 0 and stats[2] > 20 and stats[3] == 0
        assert np.bincount(match[match >= 0]).max() >= 2
    if nt == 0:
        assert stats == [0, 0, ns, 0] and mr.bits(rec).tobytes() == mr.bits(mr.transform(source, T)).tobytes()
    if ns == 0:
        assert rec.tobytes() == target.tobytes()
    held(target, source, T, RADIUS, float(mr_cos()), want=want)


def mr_cos():
    from maskfusion_amd import merge
    assert merge.COS_HALF_RAD.dtype == np.float32 and merge.COS_HALF_RAD == np.float32(np.cos(0.5))
    return merge.COS_HALF_RAD


# ---------------- crafted cases ----------------
def test_a_map_merged_into_itself_under_the_identity(hip):
    target = pool()[:257].copy()
    target[:, 3] = 8.0                                              # a power of two: (c v + c v) / (c + c) is v exactly
    for T in (None, np.eye(4)):
        rec, match, stats = want = mr.merge(target, target, T, 0.002, float(mr_cos()))
        assert stats == [257, 0, 0, 0] and np.array_equal(match, np.arange(257))
        assert rec[:, :3].tobytes() == target[:, :3].tobytes() and (rec[:, 3] == 16.0).all() and len(rec) == 257
        held(target, target, T, 0.002, float(mr_cos()), want=want)


def test_two_disjoint_maps(hip):
    target, source, T = general(257, 255)
    T = T.copy()
    T[:3, 3] += 10.0
    rec, match, stats = want = mr.merge(target, source, T, RADIUS, 0.0)
    assert stats == [0, 0, 255, 0] and (match == -1).all()
    assert rec[:257].tobytes() == target.tobytes() and rec[257:].tobytes() == mr.transform(source, T).tobytes()
    held(target, source, T, RADIUS, 0.0, want=want)


def hub_case(k, seed):
    """65 targets of which only number 40 has other surfels near it: k sources on it"""
    p = pool()
    hub = p[40]
    far = p[np.linalg.norm(p[:, :3] - hub[:3], axis=1) > 0.03]
    target = np.concatenate([far[:40], hub[None], far[40:64]])
    rng = np.random.default_rng(seed)
    return target, near(np.repeat(hub[None], k, 0), rng, sigma=0.0003)


@pytest.mark.parametrize("k", [1, 2, 7, 300])
def test_k_sources_on_one_target(hip, k):
    # the order must be under test: the case's seed is the first, counted up from 100 k, at which the restatement gives other bits when it
    # merges the list in descending order and at least one merge averages (decided on the restatement alone, before the kernel runs)
    for seed in range(100 * k, 100 * k + 50):
        target, source = hub_case(k, seed)
        rec, match, stats = want = mr.merge(target, source, None, 0.003, 0.0)
        other = mr.merge(target, source, None, 0.003, 0.0, reverse=True)[0]
        if stats[0] > 0 and (k == 1 or other[40].tobytes() != rec[40].tobytes()):
            break
    assert (match == 40).all() and stats[0] > 0 and stats[0] + stats[1] == k and stats[2:] == [0, 0] and len(rec) == 65
    if k > 1:
        assert other[40].tobytes() != rec[40].tobytes() and np.delete(other, 40, 0).tobytes() == np.delete(rec, 40, 0).tobytes()
    held(target, source, None, 0.003, 0.0, want=want)


def lone(n, spacing=1.0):
    """n well-separated targets on the x axis, facing +z"""
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = np.arange(n) * spacing
    return rsn.records(p, np.tile(np.array([0, 0, 1], np.float32), (n, 1)), confidence=3.0)


def test_the_normal_gate_at_its_threshold(hip):
    target = lone(2)
    source = target.copy()
    below = np.nextafter(F(0.8), F(0))
    source[0, 8:11] = [0.6, 0.0, F(0.8)]                             # the dot product is exactly fl(0.8): it passes
    source[1, 8:11] = [0.6, 0.0, below]                             # the float below: no partner
    rec, match, stats = want = mr.merge(target, source, None, 0.01, float(F(0.8)))
    assert match.tolist() == [0, -1] and stats == [1, 0, 1, 0] and len(rec) == 3
    held(target, source, None, 0.01, float(F(0.8)), want=want)
    assert mr.merge(target, source, None, 0.01, float(below))[1].tolist() == [0, 1]
    held(target, source, None, 0.01, float(below))


def test_a_thin_plate_finds_its_own_side(hip):
    target = lone(3)
    target[0, :3], target[0, 8:11] = [5, 0, 0.0], [0, 0, -1]        # the nearer one faces away
    target[1, :3], target[1, 8:11] = [5, 0, 0.003], [0, 0, 1]
    source = lone(1)
    source[0, :3] = [5, 0, 0.001]
    d = np.linalg.norm(target[:, :3] - source[0, :3], axis=1)
    assert d.argmin() == 0 and d[1] < 0.005
    rec, match, stats = want = mr.merge(target, source, None, 0.005, float(mr_cos()))
    assert match.tolist() == [1] and stats == [1, 0, 0, 0]
    held(target, source, None, 0.005, float(mr_cos()), want=want)
    assert mr.merge(target, source, None, 0.005, -1.0)[1].tolist() == [0]      # without the gate the back face would take it
    held(target, source, None, 0.005, -1.0)


def test_the_radius_rule_at_its_threshold(hip):
    target = lone(2)
    target[:, 11] = F(0.004)
    source = target.copy()
    source[:, :3] += F(0.0005)
    edge = F(1.5) * F(0.004)
    source[0, 11], source[1, 11] = edge, np.nextafter(edge, F(0))
    rec, match, stats = want = mr.merge(target, source, None, 0.01, 0.0)
    assert match.tolist() == [0, 1] and stats == [1, 1, 0, 0]
    assert rec[0, :3].tobytes() == target[0, :3].tobytes() and rec[0, 3] == 6.0 and rec[1, :3].tobytes() != target[1, :3].tobytes()
    held(target, source, None, 0.01, 0.0, want=want)


def test_equal_distances_go_to_the_lowest_index(hip):
    target = lone(6, spacing=10.0)
    e = 2.0 ** -10                                                  # (55 +- e and +-2 e are fp32 numbers: the distances are equal exactly)
    target[3, :3], target[1, :3] = [55 + e, 0, 0], [55 - e, 0, 0]    # 1 and 3 around x = 55
    target[4, :3], target[2, :3] = [75, -2 * e, 0], [75, 2 * e, 0]   # 2 and 4 around x = 75, the lower index on the other side
    source = lone(2)
    source[0, :3], source[1, :3] = [55, 0, 0], [75, 0, 0]
    for s, (i, j) in zip(source, ((1, 3), (2, 4))):
        d = [np.sum((s[:3] - target[m, :3]) ** 2, dtype=np.float32) for m in (i, j)]
        assert d[0] == d[1] and d[0] > 0
    rec, match, stats = want = mr.merge(target, source, None, 0.01, 0.0)
    assert match.tolist() == [1, 2]
    held(target, source, None, 0.01, 0.0, want=want)


def test_the_radius_test_at_its_threshold(hip):
    target = lone(1)
    source = lone(2)
    r = F(0.75)                                                     # r * r = 0.5625 exactly, one ulp of it is 2^-24 = (2^-12)^2
    source[0, :3], source[1, :3] = [0.75, 0, 0], [0.75, 2.0 ** -12, 0]
    d2 = source[:, 0] * source[:, 0] + source[:, 1] * source[:, 1] + source[:, 2] * source[:, 2]
    assert d2[0] == r * r and d2[1] == np.nextafter(r * r, F(1))    # exactly fl(r * r), and one ulp beyond it
    rec, match, stats = want = mr.merge(target, source, None, 0.75, 0.0)
    assert match.tolist() == [0, -1] and stats == [1, 0, 1, 0]
    held(target, source, None, 0.75, 0.0, want=want)


def test_values_that_are_not_finite_and_a_confidence_of_zero(hip):
    nan, inf = F(np.nan), F(np.inf)
    target = lone(12)
    source = target.copy()
    source[:, :3] += F(0.0005)
    source[:, 3] = 2.0
    # the target side: 0..3 are never partners and pass through; 4..7 are partners whose merge carries, but never produces, a NaN
    target[0, 0], target[1, 1], target[2, 9], target[3, 10] = nan, inf, nan, -inf
    source[0, :3], source[1, :3] = [0, 0, 0], [1, 0, 0]             # where 0 and 1 would be
    target[4, 11] = nan                                             # s.radius < NaN is false: the confidence only, the radius stays NaN
    target[5, 11] = inf                                             # averaged: the radius stays inf
    target[6, 3], source[6, 11] = inf, 1.0                          # confidence only: inf
    target[7, 3] = 0.0                                              # a target may have no confidence: the source's values come out
    # the source side: every one of these is dropped
    source[8, 2] = nan
    source[9, 8] = inf
    source[10, 3] = nan
    source[11, 3] = 0.0
    extra = source[:6].copy()
    extra[:, 0] += F(0.0001)
    extra[0, 3], extra[1, 3], extra[2, 11], extra[3, 11], extra[4, 11], extra[5, 1] = inf, -1.0, nan, inf, 0.0, -inf
    source = np.concatenate([source, extra])
    for T in (None, np.eye(4), rsn.motion()):
        s = source if T is None or np.allclose(T, np.eye(4)) else rsn.moved_records(source, np.linalg.inv(T))
        rec, match, stats = want = mr.merge(target, s, T, 0.01, 0.0)
        if T is None or np.allclose(T, np.eye(4)):
            assert match.tolist() == [-1, -1, -1, -1, 4, 5, 6, 7, -2, -2, -2, -2, -2, -2, -2, -2, -2, -2] and stats == [2, 2, 4, 10]
            assert rec[:4].tobytes() == target[:4].tobytes() and mr.bits(rec[4, 11]) == mr.bits(nan) and rec[5, 11] == inf and rec[6, 3] == inf
            assert rec[4, 3] == 5.0 and rec[7, :3].tobytes() == s[7, :3].tobytes() and rec[7, 3] == 2.0
            assert not np.isnan(np.delete(rec[4:], 0, 0)[:, [0, 1, 2, 3, 11]]).any()        # (row 4's radius is the only NaN the merges touch)
        else:
            assert stats[3] == 10 and (match[8:] == -2).all()
        held(target, s, T, 0.01, 0.0, want=want)


def test_out_capacity_one_short(hip):
    target, source, T = general(257, 255)
    rec, match, stats = mr.merge(target, source, T, RADIUS, 0.0)
    assert stats[2] > 20
    rc, out = call(target, source, T, RADIUS, 0.0, capacity=len(rec) - 1)
    assert rc == ENOMEM and out["n_out"] == len(rec) and untouched(out)
    rc, out = call(target, source, T, RADIUS, 0.0, capacity=len(rec))         # exactly enough
    assert rc == 0
    agree(out, (rec, match, stats))
    rc, out = call(target, source, T, RADIUS, 0.0, want_match=False)          # d_match is optional
    assert rc == 0 and (out["match_raw"] == SENTINEL).all() and out["records"].tobytes() == rec.tobytes()


SCHEDULE_WORKER = r'''
import hashlib, os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests"), os.path.join(%(root)r, "tests", "hipcpu")]
import emu
emu.activate()
import test_gpu_map_merge as t
target, source, T = t.general(4099, 4099)
rc, out = t.call(target, source, T, t.RADIUS, 0.0)
assert rc == 0
print(hashlib.sha256(out["records"].tobytes() + out["match"].tobytes()).hexdigest(), out["stats"])
'''


def test_two_calls_give_the_same_bytes(hip):
    target, source, T = general(4099, 4099)
    (ra, a), (rb, b) = call(target, source, T, RADIUS, 0.0), call(target, source, T, RADIUS, 0.0)
    assert ra == 0 and rb == 0 and a["stats"] == b["stats"] and a["stats"][0] > 500
    assert a["records"].tobytes() == b["records"].tobytes() and a["match"].tobytes() == b["match"].tobytes()
    mine = hashlib.sha256(a["records"].tobytes() + a["match"].tobytes()).hexdigest()
    # the CPU-executed build under the forward and the reversed thread / workgroup schedule: the same bytes, and this library's
    for schedule in (None, "reverse"):
        env = dict(os.environ)
        env.pop("HIPCPU_SCHEDULE", None)
        if schedule:
            env["HIPCPU_SCHEDULE"] = schedule
        r = subprocess.run([sys.executable, "-c", SCHEDULE_WORKER % dict(root=ROOT)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split()[0] == mine, (schedule, r.stdout)


def test_python_side(hip):
    from maskfusion_amd import merge
    target, source, T = general(257, 255)
    rec, stats, match = merge.merge_maps(target, source, T, RADIUS)
    want = mr.merge(target, source, T, RADIUS, float(mr_cos()))
    assert rec.tobytes() == want[0].tobytes() and stats == want[2] and np.array_equal(match, want[1])
    r = merge.default_radius(target)
    assert r == 2.0 * float(np.median(target[:, 11].astype(np.float64)))
    rec, stats, match = merge.merge_maps(target, source, T)
    assert rec.tobytes() == mr.merge(target, source, T, r, float(mr_cos()))[0].tobytes()
    with pytest.raises(ValueError):
        merge.merge_maps(target[:0], source)                        # no radius to derive
    rec, stats, match = merge.merge_maps(target[:0], source[:0], radius=0.01)
    assert rec.shape == (0, 12) and stats == [0, 0, 0, 0] and match.shape == (0,)


# ---------------- every MF_EINVAL of the header ----------------
def test_arguments(hip):
    from maskfusion_amd.lib import load
    L = load()
    target, source, T = general(65, 63)
    need = C.c_uint64(0)
    assert L.mf_cloud_merge_workspace(65, 63, None) == EINVAL
    for nt, ns in ((-1, 0), (0, -1), ((1 << 30) + 1, 0), (0, (1 << 30) + 1)):
        assert L.mf_cloud_merge_workspace(nt, ns, C.byref(need)) == EINVAL
    assert L.mf_cloud_merge_workspace(1 << 30, 1 << 30, C.byref(need)) == 0
    nan, inf = float("nan"), float("inf")
    bad_T = []
    for v in (nan, inf):
        B = T.copy()
        B[1, 2] = v
        bad_T.append(B)
    far_t, far_s = target.copy(), source.copy()
    far_t[7, 1] = 1e30                                              # |y / radius| >= 2^30
    far_s[9, 0] = -1e30
    cases = [dict(null=("target",)), dict(null=("source",)), dict(null=("out",)), dict(null=("n_out",)), dict(null=("stats",)), dict(null=("ws",)),
             dict(nt=(1 << 30) + 1), dict(ns=(1 << 30) + 1), dict(nt=-1), dict(ns=-1), dict(capacity=-1),
             dict(radius=0.0), dict(radius=-0.01), dict(radius=nan), dict(radius=inf),
             dict(min_cos=nan), dict(min_cos=inf), dict(min_cos=1.5), dict(min_cos=-1.5),
             dict(T=bad_T[0]), dict(T=bad_T[1]), dict(ws_short=1), dict(ws_offset=4), dict(offset=("target",)), dict(offset=("source",)),
             dict(offset=("out",)), dict(target=far_t), dict(source=far_s)]
    for kw in cases:
        args = dict(target=target, source=source, T=T, radius=RADIUS, min_cos=0.0)
        args.update(kw)
        rc, out = call(**args)
        assert rc == EINVAL and untouched(out), kw
    for kw in (dict(min_cos=1.0), dict(min_cos=-1.0), dict(T=None)):            # the ends of the range are inside it
        args = dict(target=target, source=source, T=T, radius=RADIUS, min_cos=0.0)
        args.update(kw)
        assert call(**args)[0] == 0, kw
    # a source that is dropped is not asked for its range: infinite coordinates are no overflow
    s = source.copy()
    s[9, 0] = inf
    held(target, s, T, RADIUS, 0.0)
