"""The correspondence decisions of the Gauss-Newton kernels at their boundaries (tests/gn_gate_cases.py), on every kernel that inlines them.

(A) one candidate pixel per case through k_icp_iter (mf_k_icp_step_form, form 0) at 32x24: the inlier count is the oracle's, and for an accepted
    case the 28 reduced sums are EQUAL to the oracle's -- with one inlier every sum is one fp32 product passed through additions of zero on both
    sides, and the seven row entries are claimed bit-identical (mf_gn_device.h), so equality is derived, not measured (== treats +-0 as equal).
(D) all accepted cases in one frame, all rejected ones in another (one pair per pose), at 64x48 (<256, 1>), 352x240 (<256, 2>: idle-slot skipping),
    416x296 (<512, 2>: workgroups past the image) and 520x480 (<512, 3>), through k_icp_iter, k_icp_batch_pixels without and with slab culling, and
    k_rgbd_iter: count exact, A / b / sum r^2 within test_icp_step's gates; the reject field gives 29 zeros.  The current vertices lie over the
    whole index range (first pixel, last pixel, the top slot of the last live workgroup) -- except under slab culling (form 2), whose argument is
    stated for vertex maps that are back-projections: there every vertex sits at the pixel whose ray it lies on, the model's rectangle of normals
    is the field's own, and the result must equal form 1's on the same frame, bit for bit: the culling removed nothing.
    test_slab_culling_keeps_ties_beyond_a_band: a tie that rounds one row beyond its workgroup's band, the model's rectangle being that pixel.
(B) photometric correspondences per pixel, count and sigma against the oracle; on natural derivative images the same through gate == nullptr,
    the gate image of k_derivative and the gate image of k_rgb_pyramid, the two gate images equal to each other and to numpy's.
(C) the weight's epsilon through mf_k_rgb_step.   And MF_EINVAL for thresholds icp_gates cannot bracket.

Kept out of every comparison (gn_gate_cases: the float32 projection of a finite vertex is NaN or infinite, its conversion to int undefined in every
CPU build): z_negative_zero, z_zero_on_axis, z_denormal_overflow.
Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build (tests/test_emu_gn_gates.py)."""
import functools

import numpy as np
import pytest
import torch

import gn_gate_cases as gc
from gpu_util import dev, empty, host

pytestmark = pytest.mark.gpu

CORR = np.dtype([("u0", np.int16), ("v0", np.int16), ("diff", np.float32)])
DT = (float(gc.DIST), float(gc.ANGLE))
SIZES = [(64, 48), (352, 240), (416, 296), (520, 480)]
FORMS = {(64, 48): (256, 1), (352, 240): (256, 2), (416, 296): (512, 2), (520, 480): (512, 3)}


def icp_form(hip, form, pose, K, maps, W, H, rect=None, dist=DT[0], angle=DT[1], pads=None):
    """pads: (floats in front of the model's vertex map, ... of its normal map) inside the same allocations (gn_gate_cases.row_minus_one_trap)"""
    args = [np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1)) for x in (pose.Rcurr, pose.tcurr, pose.Rpi, pose.tprev)]
    d = [dev(m) for m in maps]
    ptr = [t.data_ptr() for t in d]
    if pads is not None:
        d += [dev(np.concatenate([pads[0], maps[2].reshape(-1)])), dev(np.concatenate([pads[1], maps[3].reshape(-1)]))]
        ptr[2], ptr[3] = d[4].data_ptr() + 4 * len(pads[0]), d[5].data_ptr() + 4 * len(pads[1])
    out = empty(32)
    r = None if rect is None else np.ascontiguousarray(rect, np.int32)
    rc = hip.mf_k_icp_step_form(form, args[0].ctypes.data, args[1].ctypes.data, ptr[0], ptr[1], args[2].ctypes.data,
                                args[3].ctypes.data, *K, ptr[2], ptr[3], dist, angle, W, H, out.data_ptr(),
                                None if r is None else r.ctypes.data, None)
    return rc, host(out)


@functools.lru_cache(maxsize=None)
def _small():
    from oracle import mfo
    G, cases = gc.icp_cases()
    ref = {}
    for c in cases:
        if not c.undefined:
            maps = gc.icp_frame(G, [c])
            ref[c.name] = (c, maps, mfo.icp_step(c.pose.Rcurr, c.pose.tcurr, maps[0], maps[1], c.pose.Rpi, c.pose.tprev, *G.K(), maps[2], maps[3], *DT))
    return G, ref


CASE_NAMES = [c.name for c in gc.icp_cases()[1] if not c.undefined]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_icp_case(hip, name):
    G, ref = _small()
    c, maps, (A, b, res) = ref[name]
    assert res[1] == c.expect
    pads = None
    if name == "edge_y_below_minus_half":      # row -1: what a dropped `uy < 0` would address lies in front of the maps -- inside this test's allocation
        pad_v, pad_n, maps = gc.row_minus_one_trap(G, c, maps)
        pads = (pad_v, pad_n)
    rc, g = icp_form(hip, 0, c.pose, G.K(), maps, G.W, G.H, pads=pads)
    assert rc == 0
    assert g[28] == res[1], "the decision differs from the oracle's"
    want = gc.pack_system(A, b, res)
    if c.expect:
        assert np.array_equal(g[:29].astype(np.float64), want), np.abs(g[:29] - want).max()
    else:
        assert not g[:29].any()


@functools.lru_cache(maxsize=None)
def _fields(size, form_key, on_ray=False):
    """the four minefields of a frame size and the oracle's systems for them (computed once, read by every form)"""
    from oracle import mfo
    W, H = size
    threads, slots, blocks, chunk, live = form_key
    # a pixel of the top slot of the last live workgroup, where the image still has one; else of the last workgroup that has a full chunk
    top = (live - 1) * chunk + (slots - 1) * threads
    if top >= W * H:
        top = (live - 2) * chunk + (slots - 1) * threads
    G, fields = gc.minefields(W, H, pins=(top,), on_ray=on_ray)
    out = []
    for name, pose, cases, maps, idx, count in fields:
        out.append((name, pose, maps, idx, count, mfo.icp_step(pose.Rcurr, pose.tcurr, maps[0], maps[1], pose.Rpi, pose.tprev, *G.K(), maps[2], maps[3], *DT)))
    return G, top, out


def _launch_form(hip, W, H):
    f = np.zeros(5, np.int32)
    assert hip.mf_k_icp_launch_form(W, H, f.ctypes.data) == 0
    return tuple(int(v) for v in f)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_icp_minefields(hip, size, form):
    W, H = size
    lf = _launch_form(hip, W, H)
    threads, slots, blocks, chunk, live = lf
    assert (threads, slots) == FORMS[size]
    if size == (416, 296):
        assert live < blocks, "this size is here for its workgroups past the image"
    G, top, fields = _fields(size, lf, form == 2)
    for name, pose, maps, idx, count, (A, b, res) in fields:
        if len(idx) >= 3 and form != 2:      # the premise of the placement: the top slot and the last live workgroup carry a case
            assert any(i % chunk >= (slots - 1) * threads for i in idx) and top in idx, name
            assert any(i // chunk == live - 1 for i in idx) and idx[0] == 0 and idx[-1] == W * H - 1, name
        assert res[1] == count, name
        rect = gc.normals_rect(maps[3]) if form == 2 else None
        rc, g = icp_form(hip, form, pose, G.K(), maps, W, H, rect)
        assert rc == 0, name
        print(name, "form", form, "inliers", g[28], "expected", count)
        assert g[28] == count, name
        if count == 0:
            assert not g[:29].any(), name
            continue
        if form == 2:          # culling removed nothing: the ties that land on pixel 0 and pixel W - 2 sit at the margin it grows by
            rc1, g1 = icp_form(hip, 1, pose, G.K(), maps, W, H)
            assert rc1 == 0 and g[28] == g1[28] and np.array_equal(g, g1), name
            if pose.name == "I":    # the ties that round onto column 0 / row 0 and onto W - 2 / H - 2 put the rectangle's edges there
                assert tuple(rect) == (0, 0, W - 2, H - 2), rect
        want = gc.pack_system(A, b, res)
        gA, wA = np.zeros((6, 6)), np.zeros((6, 6))
        gb, wb = np.zeros(6), np.zeros(6)
        s = 0
        for i in range(6):
            for j in range(i, 7):
                if j == 6:
                    gb[i], wb[i] = g[s], want[s]
                else:
                    gA[i, j], wA[i, j] = g[s], want[s]
                s += 1
        scale = np.abs(wA).max()
        assert np.abs(gA - wA).max() <= 1e-4 * scale, name
        assert np.abs(gb - wb).max() <= 1e-4 * max(np.abs(wb).max(), 1e-3 * scale), name
        assert abs(g[27] - res[0]) <= 2e-5 * max(res[0], 1e-9), name


def test_slab_culling_keeps_ties_beyond_a_band(hip):
    """64x48: a vertex in the last (first) row of a workgroup's band whose tie rounds into the next (previous) row, the model's rectangle of
    normals being that one pixel: the band's projected box misses the rectangle by exactly one pixel, inside the margin the culling grows by."""
    from oracle import mfo
    W, H = 64, 48
    G, frames = gc.culling_margin_frames(W, H)
    assert len(frames) == 2 * len(range(1, H - 1, 2))
    for row, maps, rect in frames:
        res = mfo.icp_step(gc.IDENT.Rcurr, gc.IDENT.tcurr, maps[0], maps[1], gc.IDENT.Rpi, gc.IDENT.tprev, *G.K(), maps[2], maps[3], *DT)[2]
        assert res[1] == 1
        rc, g = icp_form(hip, 2, gc.IDENT, G.K(), maps, W, H, rect)
        assert rc == 0 and g[28] == 1, (row, tuple(rect))


@pytest.mark.parametrize("which", ["dist", "angle"])
@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf")])
def test_thresholds_icp_gates_cannot_bracket_are_refused(hip, which, bad):
    G, ref = _small()
    c, maps, _ = ref["dist_x_at"]
    for form in (0, 1, 3):
        rc, _ = icp_form(hip, form, c.pose, G.K(), maps, G.W, G.H, dist=bad if which == "dist" else DT[0], angle=bad if which == "angle" else DT[1])
        assert rc == -1, form
    d = [dev(m) for m in maps]
    a = [np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1)) for x in (c.pose.Rcurr, c.pose.tcurr, c.pose.Rpi, c.pose.tprev)]
    out = empty(32)
    assert hip.mf_k_icp_step(a[0].ctypes.data, a[1].ctypes.data, d[0].data_ptr(), d[1].data_ptr(), a[2].ctypes.data, a[3].ctypes.data, *G.K(),
                             d[2].data_ptr(), d[3].data_ptr(), bad if which == "dist" else DT[0], bad if which == "angle" else DT[1], G.W, G.H,
                             out.data_ptr(), None) == -1


# ---- photometric term ----
def rgb_residual(hip, minScale, dIdx, dIdy, lastDepth, nextDepth, lastImage, nextImage, kt, krk, gate=None):
    H, W = nextImage.shape
    d = [dev(np.ascontiguousarray(a)) for a in (dIdx, dIdy, lastDepth, nextDepth, lastImage, nextImage)]
    d_gate = None if gate is None else dev(np.ascontiguousarray(gate))
    cor = empty((W * H * 8,), torch.uint8)
    sums = np.zeros(2, np.int32)
    kt, krk = np.ascontiguousarray(kt, np.float32), np.ascontiguousarray(krk, np.float32)
    a = (float(minScale), *[t.data_ptr() for t in d], float(gc.DELTA), kt.ctypes.data, krk.ctypes.data, W, H, cor.data_ptr(), sums.ctypes.data)
    # without a gate through the entry the other tests use, with one through its gated form (the branch production runs)
    rc = hip.mf_k_rgb_residual(*a, None) if d_gate is None else hip.mf_k_rgb_residual_gated(*a, d_gate.data_ptr(), None)
    assert rc == 0
    return host(cor).view(CORR), int(sums[0]), int(sums[1])


def _assert_corr(got, cnt, sig, ref, name):
    cor, rsig, rcnt = ref
    valid = cor["valid"] != 0
    assert (cnt, sig) == (rcnt, rsig), name
    assert np.array_equal(got["u0"] >= 0, valid), name
    assert np.array_equal(got["u0"][valid], cor["zx"][valid]) and np.array_equal(got["v0"][valid], cor["zy"][valid]), name
    assert np.array_equal(got["diff"][valid], cor["diff"][valid]), name


RGB_NAMES = [c.name for c in gc.rgb_cases()]


@functools.lru_cache(maxsize=None)
def _rgb_small():
    from oracle import mfo_rgbd
    return {c.name: (c, mfo_rgbd.rgb_residual(float(c.minScale), c.dIdx, c.dIdy, c.lastDepth, c.nextDepth, c.lastImage, c.nextImage, c.kt, c.krk,
                                              float(gc.DELTA))) for c in gc.rgb_cases()}


@pytest.mark.parametrize("name", RGB_NAMES)
def test_rgb_case(hip, name):
    c, ref = _rgb_small()[name]
    assert ref[2] == c.expect[0]
    got, cnt, sig = rgb_residual(hip, c.minScale, c.dIdx, c.dIdy, c.lastDepth, c.nextDepth, c.lastImage, c.nextImage, c.kt, c.krk)
    _assert_corr(got, cnt, sig, ref, name)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rgb_field(hip, size):
    from oracle import mfo_rgbd
    W, H = size
    f, placed = gc.rgb_field(W, H)
    a = (f["minScale"], f["dIdx"], f["dIdy"], f["lastDepth"], f["nextDepth"], f["lastImage"], f["nextImage"], f["kt"], f["krk"])
    ref = mfo_rgbd.rgb_residual(float(a[0]), *a[1:], float(gc.DELTA))
    assert ref[2] == sum(e for _, _, e in placed)
    got, cnt, sig = rgb_residual(hip, *a)
    _assert_corr(got, cnt, sig, ref, "field")


def rgb_gate(hip, src, min_scale3):
    H, W = src.shape
    d_src = dev(src)
    g1, g2, gray = (empty((H, W), torch.uint8) for _ in range(3))
    dx, dy = empty((H, W), torch.int16), empty((H, W), torch.int16)
    ms = np.ascontiguousarray(min_scale3, np.float32)
    ran = np.zeros(1, np.int32)
    assert hip.mf_k_rgb_gate(d_src.data_ptr(), W, H, ms.ctypes.data, g1.data_ptr(), g2.data_ptr(), dx.data_ptr(), dy.data_ptr(), gray.data_ptr(),
                             ran.ctypes.data, None) == 0
    return host(g1), (host(g2) if ran[0] else None), host(dx), host(dy), (host(gray) if ran[0] else None)


@pytest.mark.parametrize("size", [(32, 24), (30, 22)] + SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rgb_gate_images_and_the_three_paths(hip, size):
    from oracle import mfo_rgbd
    W, H = size
    src = gc.texture(W, H, seed=W)
    rdx, rdy = mfo_rgbd.derivative_images(src)
    m2 = rdx.astype(np.int32) ** 2 + rdy.astype(np.int32) ** 2
    inner = m2[2:H - 3, 2:W - 7]
    vals, counts = np.unique(inner, return_counts=True)
    k = int(np.argmax(counts * (vals > 0)))
    ms = float(vals[k])                                   # the most frequent squared magnitude: many pixels sit ON the threshold
    assert counts[k] >= 3 and (inner < ms).any() and (inner > ms).any()
    g1, g2, dx, dy, gray = rgb_gate(hip, src, [ms, ms / 4, ms / 16])
    assert np.array_equal(dx, rdx) and np.array_equal(dy, rdy)
    want = gc.rgb_gate_numpy(src, dx, dy, ms)
    assert 0 < int(want.sum()) < W * H and int(((m2 == ms) & (want == 1)).sum()) >= 1
    assert np.array_equal(g1, want), int((g1 != want).sum())
    if W % 4 or H % 4:
        assert g2 is None                                 # the pyramid's tiling does not cover the size: only the first gate image
    else:
        assert np.array_equal(gray, src), "the intensity of (c, c, c) must be c for this comparison"
        assert np.array_equal(g2, g1), int((g2 != g1).sum())
    yy, xx = np.mgrid[0:H, 0:W]
    last = (1 + (xx * 7 + yy * 13) % 199).astype(np.uint8)
    depth = np.ones((H, W), np.float32)
    a = (ms, dx, dy, depth, depth, last, src, np.zeros(3, np.float32), np.eye(3, dtype=np.float32))
    ref = mfo_rgbd.rgb_residual(ms, *a[1:], float(gc.DELTA))
    assert np.array_equal(ref[0]["valid"].reshape(H, W), want)
    for gate in (None, g1, g2):
        if gate is None and g2 is None and gate is g2 and W % 4 == 0:
            continue
        if gate is g2 and g2 is None:
            continue
        got, cnt, sig = rgb_residual(hip, *a, gate=gate)
        _assert_corr(got, cnt, sig, ref, "gate" if gate is not None else "no gate")


def test_rgb_step_weight_epsilon(hip):
    from oracle import mfo_rgbd
    c = gc.weight_case()
    H, W = c.nextImage.shape
    K = (20.0, 20.0, 16.0, 12.0)
    cor, sig, cnt = mfo_rgbd.rgb_residual(float(c.minScale), c.dIdx, c.dIdy, c.lastDepth, c.nextDepth, c.lastImage, c.nextImage, c.kt, c.krk, float(gc.DELTA))
    assert cnt == 1 and sig == 0
    cloud = mfo_rgbd.project_to_cloud(c.lastDepth, *K)
    d = [dev(np.ascontiguousarray(a)) for a in (c.dIdx, c.dIdy, c.lastDepth, c.nextDepth, c.lastImage, c.nextImage)]
    d_cor = empty((W * H * 8,), torch.uint8)
    sums = np.zeros(2, np.int32)
    assert hip.mf_k_rgb_residual(float(c.minScale), *[t.data_ptr() for t in d], float(gc.DELTA), c.kt.ctypes.data,
                                 np.ascontiguousarray(c.krk).ctypes.data, W, H, d_cor.data_ptr(), sums.ctypes.data, None) == 0
    assert sums.tolist() == [1, 0]
    for name, sigma in gc.SIGMAS:
        A, b = mfo_rgbd.rgb_step(cor, float(sigma), cloud, K[0], K[1], c.dIdx, c.dIdy, W, H)
        out = np.zeros(32, np.float64)
        assert hip.mf_k_rgb_step(d_cor.data_ptr(), float(sigma), d[2].data_ptr(), *K, d[0].data_ptr(), d[1].data_ptr(), 0.125, W, H,
                                 out.ctypes.data, None) == 0
        A2 = np.zeros((6, 6)); b2 = np.zeros(6)
        k = 0
        for i in range(6):
            for j in range(i, 7):
                if j == 6: b2[i] = out[k]
                else: A2[i, j] = A2[j, i] = out[k]
                k += 1
        assert out[28] == cnt, name
        scale = np.sqrt(np.outer(np.diag(A), np.diag(A))) + 1e-30
        assert (np.abs(A2 - A) / scale).max() < 1e-5, name
        assert np.abs(b2 - b).max() <= 1e-5 * np.abs(b).max() + 1e-12, name
        assert np.abs(A).max() > 0
