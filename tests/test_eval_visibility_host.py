"""The host side of the cloud visibility in maskfusion_amd.eval, without a GPU and without the library: the numpy restatement on the literal
decision edges, cam_from_cloud, observed(), visibility_summary, compare_clouds' ref_keep (the nearest-neighbour call is replaced by a stand-in
that records its arguments) and the command's argument errors."""
import numpy as np
import pytest

import visibility_restatement as vr
import visibility_scenes as vs
from maskfusion_amd import eval as ev
from maskfusion_amd import synth


def test_restatement_on_the_literal_edges():
    points, depth, cam, want = vs.edge_inputs()
    assert len(points) == 35 and {c[3] for c in vs.edge_cases()} == {vs.OUT, vs.ON, vs.THROUGH, vs.OCC}
    for rule in (vs.EDGE_RULE, vs.EDGE_RULE_REL):
        counts, first = vr.visibility(points, depth, cam, **vs.EDGE_K, **rule)
        assert counts.dtype == np.uint32 and first.dtype == np.int32
        bad = np.flatnonzero((counts != want).any(1))
        assert bad.size == 0, [(vs.edge_cases()[i], counts[i].tolist()) for i in bad]
        assert np.array_equal(first, np.where(want[:, 1] > 0, 0, -1))
    # a hole gets no class: the same points against a depth that is not valid are in the frustum and nothing else
    for hole in (0.0, -2.0, np.nan, np.inf):
        counts, first = vr.visibility(points, np.full_like(depth, hole), cam, **vs.EDGE_K, **vs.EDGE_RULE)
        assert np.array_equal(counts[:, 0], want[:, 0]) and counts[:, 1:].sum() == 0 and (first == -1).all()
    # frame_base and accumulation: the second chunk adds, and keeps a first that is set
    counts, first = vr.visibility(points, depth, cam, **vs.EDGE_K, **vs.EDGE_RULE, frame_base=5)
    assert np.array_equal(first, np.where(want[:, 1] > 0, 5, -1))
    counts2, first2 = vr.visibility(points, depth, cam, **vs.EDGE_K, **vs.EDGE_RULE, frame_base=6, counts=counts, first=first)
    assert np.array_equal(counts2, 2 * want) and np.array_equal(first2, first)


def test_cam_from_cloud():
    poses = np.stack([synth.camera_pose(k) for k in (0, 17, 250)])
    C = synth.make_pose(synth.rot_xyz(0.3, -0.2, 1.1), [0.5, -2.0, 0.25])
    got = ev.cam_from_cloud(poses)
    assert got.dtype == np.float32 and got.shape == (3, 12) and got.flags["C_CONTIGUOUS"]
    for k, T in enumerate(poses):
        R, t = T[:3, :3], T[:3, 3]
        direct = np.concatenate([R.T, (-R.T @ t)[:, None]], 1)            # the inverse of a rigid transform, written out
        assert np.abs(got[k].reshape(3, 4) - direct).max() <= 2.0 ** -23 * max(1.0, np.abs(direct).max())
        with_cloud = (np.linalg.inv(T) @ C)[:3].astype(np.float32)
        assert np.array_equal(ev.cam_from_cloud(T, C).reshape(3, 4), with_cloud)
    assert np.array_equal(ev.cam_from_cloud(np.eye(4)), np.eye(4, dtype=np.float32)[:3].reshape(1, 12))
    assert np.array_equal(ev.cam_from_cloud(poses, C), np.concatenate([ev.cam_from_cloud(T, C) for T in poses]))


COUNTS = np.array([[0, 0, 0, 0],      # never in a frustum
                   [3, 0, 0, 0],      # in a frustum, only ever in holes
                   [4, 0, 0, 3],      # occluded in every classified frame
                   [2, 1, 0, 1],      # on the surface once
                   [5, 2, 1, 0],      # on the surface twice, seen through once
                   [2, 0, 1, 1],      # seen through once
                   [6, 0, 2, 4],      # seen through twice
                   [0, 0, 0, 0]], np.uint32)


def test_observed_rules():
    assert ev.observed(COUNTS).tolist() == [False, False, False, True, True, True, True, False]
    assert ev.observed(COUNTS, "seen", 1).tolist() == ev.observed(COUNTS).tolist()
    assert ev.observed(COUNTS, "surface").tolist() == [False, False, False, True, True, False, False, False]
    assert ev.observed(COUNTS, "seen", 2).tolist() == [False, False, False, False, True, False, True, False]
    assert ev.observed(COUNTS, "surface", 2).tolist() == [False, False, False, False, True, False, False, False]
    assert ev.observed(COUNTS, "seen", 4).sum() == 0 and ev.observed(COUNTS).dtype == np.bool_
    big = np.array([[0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0]], np.uint32)          # the sum does not wrap
    assert ev.observed(big, "seen", 2).tolist() == [True]
    for bad in (dict(rule="visible"), dict(min_frames=0)):
        with pytest.raises(ValueError):
            ev.observed(COUNTS, **bad)
    with pytest.raises(ValueError):
        ev.observed(COUNTS[:, :3])


def test_summary_categories_add_up():
    keep = ev.observed(COUNTS, "surface")
    s = ev.visibility_summary(COUNTS, keep, frames=6)
    assert s == {"frames": 6, "points": 8, "never_in_frustum": 2, "only_holes": 1, "occluded_only": 1, "reached": 4, "on_surface": 2, "seen_through": 3,
                 "kept": 2}
    assert s["never_in_frustum"] + s["only_holes"] + s["occluded_only"] + s["reached"] == len(COUNTS)
    assert ev.visibility_summary(COUNTS, ev.observed(COUNTS))["kept"] == 4 and ev.visibility_summary(COUNTS, keep)["frames"] is None
    with pytest.raises(ValueError):
        ev.visibility_summary(COUNTS, keep[:3])


def test_compare_clouds_with_and_without_a_mask(monkeypatch):
    calls = []

    def fake_nearest(target, query, radius, T=None):
        calls.append((np.array(target), np.array(query), radius, T))
        d = np.where(np.asarray(query)[:, 0] < 0.5, 0.001, np.inf).astype(np.float32)          # a query with x < 0.5 has a neighbour 1 mm away
        return d, np.zeros(len(query), np.int32)
    monkeypatch.setattr(ev, "nearest", fake_nearest)
    est = np.array([[0.0, 0, 0], [0.1, 0, 0], [0.9, 0, 0]], np.float32)
    ref = np.array([[0.0, 0, 0], [0.7, 0, 0], [0.2, 0, 0], [0.8, 0, 0], [0.3, 0, 0]], np.float32)
    old = ev.compare_clouds(est, ref, 0.05, (0.01,))
    assert len(calls) == 2
    assert np.array_equal(calls[0][0], ref) and np.array_equal(calls[0][1], est) and np.array_equal(calls[1][0], est) and np.array_equal(calls[1][1], ref)
    assert old["completeness"]["count"] == 5 and old["completeness"]["fraction"] == {"0.01": 0.6} and old["accuracy"]["fraction"] == {"0.01": 2 / 3}
    # None goes down the same path: the same calls with the same arguments, the same result
    del calls[:]
    assert ev.compare_clouds(est, ref, 0.05, (0.01,), ref_keep=None) == old
    assert len(calls) == 2 and np.array_equal(calls[1][1], ref) and calls[1][2] == 0.05 and calls[1][3] is None
    # a mask: completeness over the kept points only, accuracy against the whole reference
    del calls[:]
    keep = np.array([True, False, True, False, True])
    new = ev.compare_clouds(est, ref, 0.05, (0.01,), ref_keep=keep)
    assert np.array_equal(calls[0][0], ref) and np.array_equal(calls[1][1], ref[keep]) and np.array_equal(calls[1][0], est)
    assert new["accuracy"] == old["accuracy"] and new["completeness"]["count"] == 3 and new["completeness"]["fraction"] == {"0.01": 1.0}
    assert new["fscore"]["0.01"] == pytest.approx(2 * (2 / 3) / (2 / 3 + 1)) and set(new) == set(old)
    for bad in (keep[:4], keep.astype(np.int32)):
        with pytest.raises(ValueError):
            ev.compare_clouds(est, ref, 0.05, (0.01,), ref_keep=bad)


@pytest.mark.parametrize("args, message", [
    (["--ref-cloud", "m.ply", "--observed-poses", "p.txt"], "--observed-poses needs --observed-from"),
    (["--ref-cloud", "m.ply", "--observed-cal", "c.txt"], "--observed-cal needs --observed-from"),
    (["--ref-cloud", "m.ply", "--observed-tol", "0.01"], "--observed-tol needs --observed-from"),
    (["--ref-cloud", "m.ply", "--observed-rule", "surface"], "--observed-rule needs --observed-from"),
    (["--ref", "d", "--observed-min-frames", "2"], "--observed-min-frames needs --observed-from"),
    (["--ref", "d", "--observed-stride", "3"], "--observed-stride needs --observed-from"),
    (["--ref", "d", "--observed-max-depth", "3"], "--observed-max-depth needs --observed-from"),
    (["--gt", "g.txt", "--observed-time-scale", "1"], "--observed-time-scale needs --observed-from"),
    (["--gt", "g.txt", "--observed-from", "seq"], "--observed-from needs --ref or --ref-cloud"),
    (["--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-tol", "a"], "--observed-tol takes A or A,R"),
    (["--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-tol", "0.01,0.1,3"], "--observed-tol takes A or A,R"),
    (["--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-tol=-0.01"], "not negative"),
    (["--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-tol", "0.01,nan"], "not negative"),
    (["--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-rule", "both"], "invalid choice"),
    (["--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-min-frames", "0"], "at least 1"),
    (["--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-stride", "0"], "at least 1"),
    (["--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-max-depth", "0"], "--observed-max-depth takes"),
    (["--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-max-depth", "inf"], "--observed-max-depth takes"),
    (["--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-time-scale", "0"], "positive factor"),
])
def test_argument_errors(capsys, args, message):
    with pytest.raises(SystemExit) as e:
        ev.main(["--est", "nowhere"] + args)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_missing_pose_file_is_a_message(tmp_path, capsys):
    """--observed-from without --observed-poses needs the run's poses-0.txt: exit status 2 before anything is computed"""
    est = tmp_path / "est"
    est.mkdir()
    (est / "cloud-0.ply").write_bytes(b"")
    assert ev.main(["--est", str(est), "--ref-cloud", "m.ply", "--observed-from", "seq"]) == 2
    assert "poses-0.txt" in capsys.readouterr().err
    assert ev.main(["--est", str(est), "--ref-cloud", "m.ply", "--observed-from", "seq", "--observed-poses", str(tmp_path / "none.txt")]) == 2
    assert "--observed-poses" in capsys.readouterr().err


def test_readers_know_their_timestamps(tmp_path):
    """observe_sequence pairs frames with poses before it reads an image: both readers list the stamps of the frames they deliver"""
    from maskfusion_amd.io import readers, writers
    rgb, depth = np.zeros((6, 8, 3), np.uint8), np.full((6, 8), 1.5, np.float32)
    writers.write_image_dir(str(tmp_path / "seq"), [(rgb, depth)] * 5)
    r = readers.open_log(str(tmp_path / "seq"))
    assert r.timestamps() == [f.timestamp for f in r] and len(r.timestamps()) == 5
    for compress in (True, False):
        writers.write_klg(str(tmp_path / "a.klg"), [(1000 * k + 7, rgb, depth) for k in range(5)], compress_depth=compress)
        r = readers.open_log(str(tmp_path / "a.klg"), 8, 6)
        stamps = r.timestamps()
        assert stamps == [f.timestamp for f in r] == [7, 1007, 2007, 3007]            # the reader never delivers the last frame
        r.close()
