"""The crafted cases of tests/gn_gate_cases.py without a GPU: every premise holds, the oracle decides every case as the case expects, the oracle
agrees with the reference's own text compiled for the CPU (oracle/_ref/libmf_ref.so; skipped where that library was not built, like its other
users), and icp_gates -- the host function that turns the two ICP thresholds into boundary floats of the squared quantities, cut out of
mf_odometry.hip into tests/devmath.py's host build -- meets its definition.

Kept out of every comparison, by the rule in gn_gate_cases (the float32 projection of a finite vertex is NaN or infinite; the conversion to int is
then undefined in every CPU build): z_negative_zero, z_zero_on_axis, z_denormal_overflow."""
import time

import numpy as np
import pytest

import gn_gate_cases as gc
from oracle import mfo, mfo_rgbd, mfref

SIZES = [(32, 24), (64, 48), (352, 240), (416, 296), (520, 480)]
DT = (float(gc.DIST), float(gc.ANGLE))


def _icp(mod, pose, K, maps):
    vc, nc, vp, npv = maps
    return mod.icp_step(pose.Rcurr, pose.tcurr, vc, nc, pose.Rpi, pose.tprev, *K, vp, npv, *DT)


def _need_ref():
    if not mfref.available():
        pytest.skip("oracle/_ref/libmf_ref.so is not built and the reference is not here to build it from")


@pytest.fixture(scope="module")
def small():
    return gc.icp_cases()


def test_excluded_cases_are_the_detected_ones(small):
    G, cases = small
    assert sorted(c.name for c in cases if c.undefined) == sorted(gc.UNDEFINED_NAMES)
    listed = {"tie_x_even", "tie_x_odd", "tie_y_even", "tie_y_odd", "edge_x_minus_half", "edge_x_below_minus_half", "edge_x_size_minus_half",
              "edge_y_size_minus_half", "edge_x_size_minus_1p5", "z_negative", "z_tiny_positive", "nan_ncurr_x", "nan_ncurr_y_only", "nan_nprev_x",
              "nan_nprev_y_only", "nan_vprev", "nan_vcurr", "angle_at", "angle_below", "angle_parallel", "tie_x_even_P"}
    listed |= {f"dist_{a}_{w}" for a in "xyz" for w in ("at", "above", "below")} | {f"dist_x_{w}_P" for w in ("at", "above", "below")}
    defined = {c.name for c in cases if not c.undefined}
    assert listed <= defined


@pytest.mark.parametrize("size", SIZES)
def test_icp_premises_hold(size):
    G, cases = gc.icp_cases(*size)
    bad = [(c.name, text) for c in cases for text, ok in c.premise if not ok]
    assert not bad, bad
    assert all(c.premise for c in cases)


def test_gate_constants_are_boundaries():
    F = np.float32
    assert np.sqrt(gc.D2MAX) <= gc.DIST < np.sqrt(gc.up(gc.D2MAX))
    assert np.sqrt(gc.down(gc.S2MIN)) < gc.ANGLE <= np.sqrt(gc.S2MIN)
    assert F(gc.DIST * gc.DIST) == gc.D2MAX          # the issue's premise: 0.1f squares onto the boundary


def test_oracle_decides_each_icp_case(small):
    G, cases = small
    for c in cases:
        if c.undefined:
            continue
        A, b, res = _icp(mfo, c.pose, G.K(), gc.icp_frame(G, [c]))
        assert res[1] == c.expect, c.name


def test_reference_decides_each_icp_case(small):
    _need_ref()
    G, cases = small
    for c in cases:
        if c.undefined:
            continue
        maps = gc.icp_frame(G, [c])
        assert _icp(mfref, c.pose, G.K(), maps)[2][1] == _icp(mfo, c.pose, G.K(), maps)[2][1] == c.expect, c.name


@pytest.mark.parametrize("size", SIZES[1:])
def test_icp_minefields_oracle_and_reference(size):
    G, fields = gc.minefields(*size)
    for name, pose, cases, maps, idx, count in fields:
        A, b, res = _icp(mfo, pose, G.K(), maps)
        assert res[1] == count, name
        if count == 0:
            assert not A.any() and not b.any() and res[0] == 0
        if mfref.available():
            Ar, br, rr = _icp(mfref, pose, G.K(), maps)
            assert rr[1] == count, name
            scale = max(np.abs(A).max(), 1e-30)
            assert np.abs(Ar - A).max() <= 1e-5 * scale and np.abs(br - b).max() <= 1e-5 * scale


# ---- photometric term ----
def _residual(mod, c):
    return mod.rgb_residual(float(c.minScale), c.dIdx, c.dIdy, c.lastDepth, c.nextDepth, c.lastImage, c.nextImage, c.kt, c.krk, float(gc.DELTA))


def _check_corr_expect(cor, cnt, c):
    H, W = c.nextImage.shape
    x, y = c.px
    v = cor["valid"].reshape(H, W)
    assert cnt == c.expect[0] == int(v.sum()) and v[y, x] == c.expect[0], c.name
    if c.expect[0]:
        r = cor.reshape(H, W)[y, x]
        assert (r["zx"], r["zy"], r["ox"], r["oy"]) == (c.expect[1], c.expect[2], x, y), c.name
        assert r["diff"] == float(c.nextImage[y, x]) - float(c.lastImage[c.expect[2], c.expect[1]]), c.name


def test_rgb_premises_and_oracle_decisions():
    for c in gc.rgb_cases():
        assert all(ok for _, ok in c.premise), c.name
        cor, sig, cnt = _residual(mfo_rgbd, c)
        _check_corr_expect(cor, cnt, c)
        if c.expect[0]:
            x, y = c.px
            assert sig == int(cor.reshape(c.nextImage.shape)[y, x]["diff"] ** 2)
    big = [c for c in gc.rgb_cases() if c.name.startswith("diff_")]
    assert [abs(float(c.nextImage[10, 10]) - float(c.lastImage[10, 10])) for c in big] == [254.0, 254.0]


def _same_corr(a, b, name):
    """valid per pixel; the other fields where valid (the reference leaves them unwritten elsewhere)"""
    assert np.array_equal(a["valid"], b["valid"]), name
    m = a["valid"] != 0
    for k in ("zx", "zy", "ox", "oy", "diff"):
        assert np.array_equal(a[k][m], b[k][m]), (name, k)


def test_rgb_reference_matches_oracle():
    _need_ref()
    for c in gc.rgb_cases():
        co, so, no = _residual(mfo_rgbd, c)
        cr, sr, nr = _residual(mfref, c)
        _same_corr(co, cr, c.name)
        assert (no, so) == (nr, sr), c.name


@pytest.mark.parametrize("size", SIZES[1:])
def test_rgb_field_oracle_and_reference(size):
    W, H = size
    f, placed = gc.rgb_field(W, H)
    args = (float(f["minScale"]), f["dIdx"], f["dIdy"], f["lastDepth"], f["nextDepth"], f["lastImage"], f["nextImage"], f["kt"], f["krk"], float(gc.DELTA))
    cor, sig, cnt = mfo_rgbd.rgb_residual(*args)
    v = cor["valid"].reshape(H, W)
    for name, (x, y), e in placed:
        assert v[y, x] == e, name
    assert cnt == int(v.sum()) == sum(e for _, _, e in placed)
    if mfref.available():
        cr, sr, nr = mfref.rgb_residual(*args)
        _same_corr(cor, cr, "field")
        assert (cnt, sig) == (nr, sr)


def test_rgb_step_weights_oracle_and_reference():
    c = gc.weight_case()
    H, W = c.nextImage.shape
    cor, sig, cnt = _residual(mfo_rgbd, c)
    assert cnt == 1 and sig == 0 and cor[cor["valid"] != 0]["diff"][0] == 0
    K = (20.0, 20.0, 16.0, 12.0)
    cloud = mfo_rgbd.project_to_cloud(c.lastDepth, *K)
    got = {}
    for name, s in gc.SIGMAS:
        A, b = mfo_rgbd.rgb_step(cor, float(s), cloud, K[0], K[1], c.dIdx, c.dIdy, W, H)
        got[name] = A
        assert not b.any()                                  # row[6] = -w diff = 0
        if mfref.available():
            Ar, br = mfref.rgb_step(cor, float(s), mfref.project_to_cloud(c.lastDepth, *K), K[0], K[1], c.dIdx, c.dIdy, W, H)
            assert np.abs(Ar - A).max() <= 1e-5 * np.abs(A).max() and not br.any(), name
    # w = 1 for sigma 0, for sigma == epsilon (not greater) and for -1; 1 / nextafter(epsilon) just above it: A scales with w^2
    assert np.array_equal(got["zero"], got["epsilon"]) and np.array_equal(got["zero"], got["minus_one"])
    w = 1.0 / float(gc.up(gc.EPS))
    assert 8.3e6 < w < 8.4e6 and np.allclose(got["above_epsilon"], got["zero"] * w * w, rtol=1e-5)


# ---- icp_gates ----
def _thresholds():
    F = np.float32
    fixed = [F(0.10), gc.ANGLE, F(0), F(1e-20), np.nextafter(F(0), F(1)), F(1e19), np.finfo(F).max]
    rng = np.random.default_rng(20)
    return fixed, np.exp(rng.uniform(np.log(1e-3), np.log(10.0), 1000)).astype(F)


def test_icp_gates_meet_their_definition():
    import devmath
    L = devmath.lib()
    fixed, seeded = _thresholds()
    out = np.zeros(2, np.float32)
    pairs = [(t, s) for t in fixed for s in fixed] + list(zip(seeded, seeded[::-1]))
    with np.errstate(over="ignore"):
        for T, S in pairs:
            t0 = time.perf_counter()
            L.dm_icp_gates(float(T), float(S), out)
            assert time.perf_counter() - t0 < 1.0, (T, S)
            d2, s2 = out
            assert np.sqrt(d2) <= T < np.sqrt(gc.up(d2)), (T, d2)
            assert (s2 == 0 and S == 0) or (np.sqrt(gc.down(s2)) < S <= np.sqrt(s2)), (S, s2)
    L.dm_icp_gates(float(gc.DIST), float(gc.ANGLE), out)
    assert out[0] == gc.D2MAX and out[1] == gc.S2MIN
