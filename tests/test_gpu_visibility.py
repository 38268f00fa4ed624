"""Cloud visibility on the device: mf_cloud_visibility_dev against the numpy restatement of its definition (tests/visibility_restatement.py),
the Visibility accumulator, observed(), compare_clouds' ref_keep and the command's --observed-* flags.  Every output is an integer and every
comparison is exact equality on all four counters and on d_first.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build."""
import json
import math

import numpy as np
import pytest

import visibility_restatement as vr
import visibility_scenes as vs

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
EINVAL = -1


def _dev(a):
    import torch
    from maskfusion_amd.lib import torch_device
    return torch.as_tensor(np.array(a, order="C")).to(torch_device())          # a copy: the scenes are read-only


def _sync(t):
    import torch
    if t.device.type == "cuda":
        torch.cuda.synchronize()


def _outputs(n, fill=0xA5):
    """(counts, first) device tensors for n points, every byte `fill`"""
    import torch
    from maskfusion_amd.lib import torch_device
    word = int(np.array([fill] * 4, np.uint8).view(np.int32)[0])
    return (torch.full((max(n, 1), 4), word, dtype=torch.int32, device=torch_device()), torch.full((max(n, 1),), word, dtype=torch.int32, device=torch_device()))


def _call(t_points, t_depth, t_cam, k, rule, t_counts, t_first, frame_base=0, accumulate=0, **over):
    """the raw library call on device tensors; `over` replaces single arguments"""
    from maskfusion_amd.lib import load
    a = dict(points=t_points.data_ptr(), stride=int(t_points.shape[1]), n=int(t_points.shape[0]), depth=t_depth.data_ptr(), cam=t_cam.data_ptr(),
             n_frames=int(t_depth.shape[0]), height=int(t_depth.shape[1]), width=int(t_depth.shape[2]), frame_base=frame_base, accumulate=accumulate,
             counts=t_counts.data_ptr(), first=t_first.data_ptr())
    a.update(k)
    a.update(rule)
    a.update(over)
    return load().mf_cloud_visibility_dev(a["points"], a["stride"], a["n"], a["depth"], a["cam"], a["n_frames"], a["height"], a["width"], a["fx"], a["fy"], a["cx"],
                                          a["cy"], a["near_z"], a["far_z"], a["tol_abs"], a["tol_rel"], a["frame_base"], a["accumulate"], a["counts"], a["first"], None)


def _run(points, depth, cam, k, rule, **kw):
    """one call into 0xA5-filled outputs -> (counts uint32 (n, 4), first int32 (n,)) as numpy"""
    tp, td, tc = _dev(points), _dev(depth), _dev(cam)
    counts, first = _outputs(len(points))
    assert _call(tp, td, tc, k, rule, counts, first, **kw) == 0
    _sync(counts)
    n = len(points)
    return counts[:n].cpu().numpy().view(np.uint32), first[:n].cpu().numpy()


def _same(got, want):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]), np.flatnonzero((got[0] != want[0]).any(1))[:10]
    assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])[:10]


@pytest.fixture(scope="module")
def random_want():
    """the restatement's result for the random cloud over its first five frames, computed once"""
    p, d, cam = vs.random_cloud()
    want = vr.visibility(p, d[:5], cam[:5], **vs.RANDOM_K, **vs.RANDOM_RULE)
    for a in want:
        a.setflags(write=False)
    return want


# ---------------------------------------------------------------- the rule ----------------------------------------------------------------
def test_random_cloud_exercises_every_branch(random_want):
    """before the library is trusted with it: the cloud has points that are never in a frustum, and at least 20 classifications of each kind"""
    c = random_want[0].astype(np.int64)
    holes = int(c[:, 0].sum() - c[:, 1:].sum())
    print("never in a frustum", int((c[:, 0] == 0).sum()), "holes", holes, "on", int(c[:, 1].sum()), "through", int(c[:, 2].sum()), "occluded", int(c[:, 3].sum()))
    assert (c[:, 0] == 0).sum() >= 20 and holes >= 20 and c[:, 1].sum() >= 20 and c[:, 2].sum() >= 20 and c[:, 3].sum() >= 20
    assert set(random_want[1].tolist()) == {-1, 0, 1, 3, 4}          # d_first takes every value it can: nothing is on the sheet of frame 2


@pytest.mark.parametrize("stride", [3, 4, 12])
def test_random_cloud_equals_restatement(hip, random_want, stride):
    p, d, cam = vs.random_cloud()
    _same(_run(p[:, :stride], d[:5], cam[:5], vs.RANDOM_K, vs.RANDOM_RULE), random_want)


def test_no_far_limit(hip):
    """FLT_MAX and +inf both mean no limit: the points far outside are classified like the rest"""
    p, d, cam = vs.random_cloud()
    want = vr.visibility(p, d[:5], cam[:5], **vs.RANDOM_K, **dict(vs.RANDOM_RULE, far_z=np.inf))
    for far in (FLT_MAX, math.inf):
        _same(_run(p[:, :3], d[:5], cam[:5], vs.RANDOM_K, dict(vs.RANDOM_RULE, far_z=far)), want)


def test_decision_edges(hip):
    """every border of the rule hit exactly and missed by one float; the expected class is a literal (visibility_scenes.edge_cases) and the
    restatement agrees with it"""
    points, depth, cam, want = vs.edge_inputs()
    first = np.where(want[:, 1] > 0, 0, -1).astype(np.int32)
    for rule in (vs.EDGE_RULE, vs.EDGE_RULE_REL):          # the same two edges through tol_abs, and through the product tol_rel * d
        re_c, re_f = vr.visibility(points, depth, cam, **vs.EDGE_K, **rule)
        assert np.array_equal(re_c, want) and np.array_equal(re_f, first), "the restatement and the literals disagree"
        _same(_run(points, depth, cam, vs.EDGE_K, rule), (want, first))


# ---------------------------------------------------------------- chunks, sizes, purity ----------------------------------------------------------------
def test_chunks_equal_one_call(hip):
    """seven frames as 3 + 4 with accumulate and frame_base; the first call overwrites buffers full of 0xA5"""
    p, d, cam = vs.random_cloud()
    p = p[:, :3]
    want = vr.visibility(p, d, cam, **vs.RANDOM_K, **vs.RANDOM_RULE)
    assert (want[1] >= 5).sum() >= 1, "some point must be on the surface for the first time in the second chunk"
    _same(_run(p, d, cam, vs.RANDOM_K, vs.RANDOM_RULE), want)
    tp, td, tc = _dev(p), _dev(d), _dev(cam)
    counts, first = _outputs(len(p))
    assert _call(tp, td[:3], tc[:3], vs.RANDOM_K, vs.RANDOM_RULE, counts, first) == 0
    _sync(counts)
    part = (counts.cpu().numpy().view(np.uint32).copy(), first.cpu().numpy().copy())      # (off the GPU, .cpu() is the tensor itself)
    _same(part, vr.visibility(p, d[:3], cam[:3], **vs.RANDOM_K, **vs.RANDOM_RULE))
    assert (part[0] < 0xA5).all() and (part[1] < 0xA5).all(), "nothing of the fill is left"
    assert _call(tp, td[3:].contiguous(), tc[3:].contiguous(), vs.RANDOM_K, vs.RANDOM_RULE, counts, first, frame_base=3, accumulate=1) == 0
    _sync(counts)
    _same((counts.cpu().numpy().view(np.uint32), first.cpu().numpy()), want)
    # and the restatement's own accumulation says the same
    _same(vr.visibility(p, d[3:], cam[3:], **vs.RANDOM_K, **vs.RANDOM_RULE, frame_base=3, counts=part[0], first=part[1]), want)


def test_accumulator_in_chunks(hip):
    """Visibility.add() three times equals the single call, from numpy points and from a device tensor"""
    from maskfusion_amd import eval as ev
    p, d, cam = vs.random_cloud()
    want = vr.visibility(p, d, cam, **vs.RANDOM_K, **vs.RANDOM_RULE)
    R = vs.RANDOM_RULE
    for points in (p, _dev(p[:, :4])):
        v = ev.Visibility(points, near=R["near_z"], far=R["far_z"], tol_abs=R["tol_abs"], tol_rel=R["tol_rel"], **vs.RANDOM_K)
        v.add(d[:2], cam[:2])
        v.add(d[2], cam[2])
        v.add(_dev(d[3:]), cam[3:])
        assert v.frames == 7
        _same(v.result(), want)
    empty = ev.Visibility(np.zeros((0, 3), np.float32), **vs.RANDOM_K)
    empty.add(d[:2], cam[:2])
    got = empty.result()
    assert got[0].shape == (0, 4) and got[1].shape == (0,)


@pytest.mark.parametrize("n_frames", [1, 2])
@pytest.mark.parametrize("n", [1, 64, 65, 256, 257])
def test_sizes(hip, n, n_frames):
    p, d, cam = vs.random_cloud()
    sel = p[100:100 + n, :3]               # back-projected points: they are classified
    want = vr.visibility(sel, d[:n_frames], cam[:n_frames], **vs.RANDOM_K, **vs.RANDOM_RULE)
    assert want[0][:, 0].sum() > 0
    _same(_run(sel, d[:n_frames], cam[:n_frames], vs.RANDOM_K, vs.RANDOM_RULE), want)


def test_counts_need_no_alignment(hip):
    """d_counts 4 bytes past a 16-byte boundary, with and without accumulate"""
    import torch
    p, d, cam = vs.random_cloud()
    p = p[:, :3]
    want = vr.visibility(p, d, cam, **vs.RANDOM_K, **vs.RANDOM_RULE)
    tp, td, tc = _dev(p), _dev(d), _dev(cam)
    big, first = torch.zeros(len(p) * 4 + 8, dtype=torch.int32, device=tp.device), _outputs(len(p))[1]
    off = ((-big.data_ptr()) % 16) // 4 + 1
    counts = big[off:off + len(p) * 4].view(len(p), 4)
    assert counts.data_ptr() % 16 == 4
    assert _call(tp, td[:3], tc[:3], vs.RANDOM_K, vs.RANDOM_RULE, counts, first) == 0
    assert _call(tp, td[3:].contiguous(), tc[3:].contiguous(), vs.RANDOM_K, vs.RANDOM_RULE, counts, first, frame_base=3, accumulate=1) == 0
    _sync(counts)
    _same((counts.cpu().numpy().view(np.uint32), first.cpu().numpy()), want)
    assert big[:off].abs().sum() == 0 and big[off + len(p) * 4:].abs().sum() == 0


def test_no_points(hip):
    p, d, cam = vs.random_cloud()
    tp, td, tc = _dev(p), _dev(d), _dev(cam)
    counts, first = _outputs(4)
    assert _call(tp, td, tc, vs.RANDOM_K, vs.RANDOM_RULE, counts, first, n=0) == 0
    assert _call(tp, td, tc, vs.RANDOM_K, vs.RANDOM_RULE, counts, first, n=0, points=None, counts=None, first=None) == 0
    _sync(counts)
    assert (counts.cpu().numpy().view(np.uint8) == 0xA5).all() and (first.cpu().numpy().view(np.uint8) == 0xA5).all()


def test_purity(hip):
    """two calls give identical outputs; points, depth and poses are bit-identical afterwards"""
    p, d, cam = vs.random_cloud()
    tp, td, tc = _dev(p), _dev(d), _dev(cam)
    res = []
    for fill in (0xA5, 0x11):
        counts, first = _outputs(len(p), fill)
        assert _call(tp, td, tc, vs.RANDOM_K, vs.RANDOM_RULE, counts, first) == 0
        _sync(counts)
        res.append((counts.cpu().numpy().copy(), first.cpu().numpy().copy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    for t, a in ((tp, p), (td, d), (tc, cam)):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def test_argument_checks(hip):
    """every refused call returns MF_EINVAL and leaves the 0xA5-filled outputs untouched"""
    p, d, cam = vs.random_cloud()
    tp, td, tc = _dev(p), _dev(d), _dev(cam)
    counts, first = _outputs(len(p))
    call = lambda **k: _call(tp, td, tc, vs.RANDOM_K, vs.RANDOM_RULE, counts, first, **k)
    nan, inf = float("nan"), float("inf")
    for key in ("points", "depth", "cam", "counts", "first"):
        assert call(**{key: None}) == EINVAL, key
    assert call(stride=2) == EINVAL and call(stride=0) == EINVAL and call(stride=-3) == EINVAL
    assert call(n=(1 << 30) + 1) == EINVAL and call(n=-1) == EINVAL
    for key in ("n_frames", "width", "height"):
        assert call(**{key: 0}) == EINVAL and call(**{key: -2}) == EINVAL, key
    assert call(width=4097, height=4096) == EINVAL and call(width=1 << 16, height=1 << 16) == EINVAL      # the second: W H wraps an int32
    for key in ("fx", "fy"):
        for v in (0.0, nan, inf, -inf):
            assert call(**{key: v}) == EINVAL, (key, v)
    for key in ("cx", "cy"):
        for v in (nan, inf, -inf):
            assert call(**{key: v}) == EINVAL, (key, v)
    for v in (0.0, -0.5, nan, inf):
        assert call(near_z=v) == EINVAL, v
    for v in (vs.RANDOM_RULE["near_z"], 0.01, -1.0, nan):
        assert call(far_z=v) == EINVAL, v
    for key in ("tol_abs", "tol_rel"):
        for v in (-1e-9, nan, inf, -inf):
            assert call(**{key: v}) == EINVAL, (key, v)
    assert call(frame_base=-1) == EINVAL
    _sync(counts)
    assert (counts.cpu().numpy().view(np.uint8) == 0xA5).all() and (first.cpu().numpy().view(np.uint8) == 0xA5).all()
    # nothing was launched, nothing is broken: a valid call still succeeds (negative fx, zero tolerances and cx outside the image are valid)
    assert call(fx=-33.0, tol_abs=0.0, tol_rel=0.0, cx=-5.0) == 0
    _sync(counts)
    want = vr.visibility(p, d, cam, **dict(vs.RANDOM_K, fx=-33.0, cx=-5.0), **dict(vs.RANDOM_RULE, tol_abs=0.0, tol_rel=0.0))
    _same((counts.cpu().numpy().view(np.uint32), first.cpu().numpy()), want)


# ---------------------------------------------------------------- the crafted scene ----------------------------------------------------------------
def _crafted_counts(ev, ref, depth, poses, rule):
    v = ev.Visibility(ref, near=rule["near_z"], far=rule["far_z"], tol_abs=rule["tol_abs"], tol_rel=rule["tol_rel"], **vs.CRAFT_K)
    v.add(depth, ev.cam_from_cloud(poses))
    return v.result()


def test_crafted_scene(hip):
    """a reference of which the four frames saw exactly the first 19 200 points: the culled completeness is 1, the plain one 19 200 / 20 200"""
    from maskfusion_amd import eval as ev
    frames, poses, ref = vs.crafted()
    depth = np.stack([f[1] for f in frames])
    S = vs.CRAFT_SEEN
    assert ref.shape == (S + 1000, 3)
    counts, first = _crafted_counts(ev, ref, depth, poses, vs.CRAFT_RULE)
    _same((counts, first), vr.visibility(ref, depth, ev.cam_from_cloud(poses), **vs.CRAFT_K, **vs.CRAFT_RULE))
    assert (counts[:S, 1] >= 1).all()                                             # every seen point is on the surface in at least one frame
    assert (first[:S] >= 0).all() and (first[:S // 4] == 0).all() and (first[S:] == -1).all()      # frame 0's own pixels are on its surface
    wall = counts[S:S + 500]
    assert wall[:, 1].sum() == 0 and wall[:, 2].sum() == 0                        # behind the wall: never on it, never seen through
    assert np.count_nonzero((wall[:, 0] > 0) & (wall[:, 3] == wall[:, 0])) == 496   # 496 of the 500 are in a frustum, and occluded there
    assert counts[S + 500:, 0].sum() == 0                                         # behind every camera: in no frustum
    for rule in ("seen", "surface"):
        assert np.array_equal(np.flatnonzero(ev.observed(counts, rule)), np.arange(S)), rule
    keep = ev.observed(counts)
    s = ev.visibility_summary(counts, keep, 4)
    assert s["kept"] == S and s["never_in_frustum"] + s["only_holes"] + s["occluded_only"] + s["reached"] == len(ref) and s["frames"] == 4
    assert s["occluded_only"] == 496 and s["never_in_frustum"] == 504 and s["reached"] == S
    est = ref[:S]
    culled = ev.compare_clouds(est, ref, ref_keep=keep)
    plain = ev.compare_clouds(est, ref)
    assert culled["completeness"]["count"] == S and all(v == 1.0 for v in culled["completeness"]["fraction"].values())
    assert plain["completeness"]["count"] == S + 1000 and all(v == S / (S + 1000) for v in plain["completeness"]["fraction"].values())
    assert culled["accuracy"] == plain["accuracy"] and plain == ev.compare_clouds(est, ref, ref_keep=None)
    assert all(culled["fscore"][k] == 1.0 and plain["fscore"][k] < 1.0 for k in culled["fscore"])


# ---------------------------------------------------------------- the command ----------------------------------------------------------------
def _write_ply(path, xyz):
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(xyz)).encode())
        f.write(np.ascontiguousarray(xyz, "<f4").tobytes())


def _quaternion(R):
    """(qx, qy, qz, qw) of a rotation near the identity"""
    w = math.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 2.0
    return (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w


def test_command(hip, tmp_path, capsys):
    """the crafted scene as a sequence directory (16-bit millimetre depth), an export directory and a reference PLY"""
    from maskfusion_amd import eval as ev
    from maskfusion_amd.io import readers, writers
    frames, poses, _ = vs.crafted()
    seq, est = tmp_path / "seq", tmp_path / "est"
    est.mkdir()
    writers.write_image_dir(str(seq), frames, calibration=(*vs.CRAFT_K.values(), vs.CRAFT_W, vs.CRAFT_H))
    reader = readers.open_log(str(seq))
    stamps = reader.timestamps()
    depth = [reader.load(k).depth for k in range(len(frames))]                    # the quantised depth the command will read
    assert len(stamps) == 4 and all(np.abs(d - f[1]).max() <= 0.00051 for d, f in zip(depth, frames))
    ref = vs.crafted_from(depth, poses)
    S = vs.CRAFT_SEEN
    scale = 1e-3                                                                   # the image reader stamps in milliseconds
    with open(est / "poses-0.txt", "w") as f:
        for t, T in zip(stamps, poses):
            f.write("%.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f\n" % (t * scale, *T[:3, 3], *_quaternion(T[:3, :3])))
    # the 5 mm tolerance covers the pose file's six decimals: on the restatement, with the poses as the command reads them
    log = ev.read_tum(str(est / "poses-0.txt"))
    c, _ = vr.visibility(ref, np.stack(depth), ev.cam_from_cloud(log[1]), **vs.CRAFT_K, near_z=ev.OBSERVED_NEAR, far_z=np.inf, tol_abs=0.005, tol_rel=0.0)
    assert np.array_equal(np.flatnonzero(ev.observed(c)), np.arange(S))
    _write_ply(est / "cloud-0.ply", ref[:S])
    _write_ply(tmp_path / "ref.ply", ref)
    base = ["--est", str(est), "--ref-cloud", str(tmp_path / "ref.ply")]
    assert ev.main(base) == 0
    plain = json.loads(capsys.readouterr().out)
    assert ev.main(base + ["--observed-from", str(seq), "--observed-cal", str(seq / "calibration.txt"), "--observed-tol", "0.005",
                           "--observed-time-scale", str(scale)]) == 0
    o = json.loads(capsys.readouterr().out)
    assert o["observed"]["kept"] == S and o["observed"]["frames"] == 4 and o["observed"]["frames_skipped"] == 0 and o["observed"]["rule"] == "seen"
    assert o["observed"]["points"] == S + 1000 and o["observed"]["tol_abs"] == 0.005 and o["observed"]["tol_rel"] == 0.0
    assert all(v == 1.0 for v in o["cloud_observed"]["completeness"]["fraction"].values()) and o["cloud_observed"]["completeness"]["count"] == S
    assert all(v < 1.0 for v in o["cloud"]["completeness"]["fraction"].values())
    assert o["cloud"] == plain["cloud"] and set(o) == set(plain) | {"observed", "cloud_observed"}
    # every second frame, and a time scale under which no frame has a pose
    assert ev.main(base + ["--observed-from", str(seq), "--observed-cal", str(seq / "calibration.txt"), "--observed-time-scale", str(scale),
                           "--observed-stride", "2"]) == 0
    o2 = json.loads(capsys.readouterr().out)
    assert o2["observed"]["frames"] == 2 and 0 < o2["observed"]["kept"] < S
    with open(tmp_path / "late.txt", "w") as f:
        f.write("".join("1" + line for line in open(est / "poses-0.txt")))          # every timestamp ten seconds or more later
    assert ev.main(base + ["--observed-from", str(seq), "--observed-cal", str(seq / "calibration.txt"), "--observed-time-scale", str(scale),
                           "--observed-poses", str(tmp_path / "late.txt")]) == 2
    assert "has a pose" in capsys.readouterr().err
