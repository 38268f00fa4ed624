"""The host side of the cloud normals in maskfusion_amd.eval, without a GPU: the command's argument errors, normal_consistency's numpy part
on hand-made pairs, and --estimate-normals left unused for a reference PLY that carries normals (the device calls are replaced by
stand-ins that record their use)."""
import json
import math

import numpy as np
import pytest

from maskfusion_amd import eval as ev


def _write_ply(path, xyz, nrm=None):
    props = "property float x\nproperty float y\nproperty float z\n" + ("property float nx\nproperty float ny\nproperty float nz\n" if nrm is not None else "")
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%send_header\n" % (len(xyz), props)).encode())
        f.write(np.ascontiguousarray(xyz if nrm is None else np.concatenate([xyz, nrm], 1), "<f4").tobytes())


@pytest.mark.parametrize("args, message", [
    (["--gt", "g.txt", "--estimate-normals"], "need --ref or --ref-cloud"),
    (["--gt", "g.txt", "--normals"], "need --ref or --ref-cloud"),
    (["--seg-gt", "d", "--estimate-normals=0.1"], "need --ref or --ref-cloud"),
    (["--ref-cloud", "m.ply", "--estimate-normals=0"], "positive radius"),
    (["--ref-cloud", "m.ply", "--estimate-normals=-0.1"], "positive radius"),
    (["--ref-cloud", "m.ply", "--estimate-normals=nan"], "positive radius"),
    (["--ref-cloud", "m.ply", "--estimate-normals=x"], "invalid float value"),
])
def test_argument_errors(capsys, args, message):
    with pytest.raises(SystemExit) as e:
        ev.main(["--est", "nowhere"] + args)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_normal_angles_on_hand_made_pairs():
    z = [0.0, 0.0, 1.0]
    est = np.array([z, z, [0.0, 0.0, -2.0], [1.0, 0.0, 0.0], [0.0, math.sin(math.radians(20)), math.cos(math.radians(20))], [np.nan, 0.0, 0.0], z])
    ref = np.array([z, [0.0, 3.0, 0.0], [np.nan, np.nan, np.nan]])
    idx = np.array([0, 1, 0, 0, 0, 0, 2])
    ang = ev.normal_angles(est, ref, idx)
    assert ang.shape == (5,)                                     # a NaN normal on either side drops the pair
    assert np.abs(ang - [0.0, 90.0, 0.0, 90.0, 20.0]).max() < 1e-12      # the sign and the length of a normal do not matter
    assert ev.normal_angles(est, ref, np.full(7, -1)).size == 0          # no partner, no pair
    # T turns the est normals: a quarter turn about x takes y to z
    T = np.eye(4)
    T[:3, :3] = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
    T[:3, 3] = [5.0, 6.0, 7.0]
    assert abs(ev.normal_angles([[0.0, 1.0, 0.0]], [z], [0], T)[0]) < 1e-12
    assert abs(ev.normal_angles([[0.0, 1.0, 0.0]], [z], [0])[0] - 90.0) < 1e-12


def test_normal_consistency_summary(monkeypatch):
    idx = np.array([0, 1, 2, -1, 3], np.int32)
    monkeypatch.setattr(ev, "nearest", lambda ref, est, radius, T=None: (np.zeros(len(idx), np.float32), idx))
    deg = np.radians([4.0, 12.0, 25.0, 0.0, 50.0])
    est_n = np.stack([np.zeros(5), np.sin(deg), np.cos(deg)], 1)
    ref_n = np.tile([0.0, 0.0, 1.0], (4, 1))
    res = ev.normal_consistency(np.zeros((5, 3), np.float32), est_n, np.zeros((4, 3), np.float32), ref_n, 0.05)
    assert res["radius"] == 0.05 and res["count"] == 5 and res["pairs"] == 4
    assert abs(res["mean_deg"] - (4 + 12 + 25 + 50) / 4) < 1e-9 and abs(res["median_deg"] - 18.5) < 1e-9
    assert res["below"] == {"10": 0.25, "20": 0.5, "30": 0.75}
    monkeypatch.setattr(ev, "nearest", lambda ref, est, radius, T=None: (np.zeros(2, np.float32), np.array([-1, -1], np.int32)))
    res = ev.normal_consistency(np.zeros((2, 3), np.float32), est_n[:2], np.zeros((4, 3), np.float32), ref_n, 0.05)
    assert res["pairs"] == 0 and res["mean_deg"] is None and res["median_deg"] is None and res["below"] == {"10": 0.0, "20": 0.0, "30": 0.0}


def test_estimate_normals_is_unused_for_a_ply_with_normals(monkeypatch, tmp_path, capsys):
    rng = np.random.default_rng(1)
    xyz = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (50, 1))
    est = tmp_path / "est"
    est.mkdir()
    _write_ply(str(est / "cloud-0.ply"), xyz, nrm)
    _write_ply(str(tmp_path / "with.ply"), xyz, nrm)
    _write_ply(str(tmp_path / "bare.ply"), xyz)
    calls = []
    monkeypatch.setattr(ev, "compare_clouds", lambda *a, **k: {"stub": True})
    monkeypatch.setattr(ev, "nearest", lambda ref, e, radius, T=None: (np.zeros(len(e), np.float32), np.arange(len(e), dtype=np.int32)))

    def fake_estimate(points, radius, min_neighbours=5, viewpoint=None):
        calls.append((len(points), radius, viewpoint))
        out = np.tile(np.array([[0, 1, 0]], np.float32), (len(points), 1))
        out[:3] = np.nan
        return out, np.zeros(len(points), np.float32), np.full(len(points), 9, np.int32)
    monkeypatch.setattr(ev, "estimate_normals", fake_estimate)
    base = ["--est", str(est), "--radius", "0.03"]
    # the file's normals are used as they are
    assert ev.main(base + ["--ref-cloud", str(tmp_path / "with.ply"), "--estimate-normals", "--normals"]) == 0
    o = json.loads(capsys.readouterr().out)
    assert calls == [] and "reference_normals" not in o and o["normal_consistency"]["median_deg"] == 0.0 and o["normal_consistency"]["pairs"] == 50
    # a file without: estimated with no viewpoint at twice --radius, and recorded
    assert ev.main(base + ["--ref-cloud", str(tmp_path / "bare.ply"), "--estimate-normals", "--normals"]) == 0
    o = json.loads(capsys.readouterr().out)
    assert calls == [(50, 0.06, None)] and o["reference_normals"] == {"estimated": True, "radius": 0.06, "without_normal": 3}
    assert o["normal_consistency"]["pairs"] == 47 and o["normal_consistency"]["median_deg"] == 90.0
    # neither flag: nothing of all this in the output
    assert ev.main(base + ["--ref-cloud", str(tmp_path / "bare.ply")]) == 0
    assert json.loads(capsys.readouterr().out) == {"model": 0, "ref_cloud": str(tmp_path / "bare.ply"), "cloud": {"stub": True}}
    assert len(calls) == 1
    # --normals alone with a bare reference: no normals on one side, no entry
    assert ev.main(base + ["--ref-cloud", str(tmp_path / "bare.ply"), "--normals"]) == 0
    assert "normal_consistency" not in json.loads(capsys.readouterr().out)
