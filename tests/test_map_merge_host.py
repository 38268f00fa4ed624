"""The host side of map merging (maskfusion_amd.merge: the constants, the stamp rewrite, the arguments of the command and its errors) with the
device call replaced by its numpy restatement (tests/merge_restatement.py), and the restatement's own sanity.  No GPU."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_restatement as mr  # noqa: E402
import redetect_scene as rsn  # noqa: E402
from maskfusion_amd import merge  # noqa: E402


def stand_in(target, source, T=None, radius=None, min_cos=merge.COS_HALF_RAD):
    """merge.merge_maps's signature and order of results, computed by the restatement"""
    rec, match, stats = mr.merge(target, source, T, merge.default_radius(target) if radius is None else radius, float(min_cos))
    return rec, stats, match


def maps(n=300):
    obj = rsn.object_records(2000, seed=5)
    rng = np.random.default_rng(2)
    a = obj[rng.permutation(len(obj))[:n]].copy()
    b = a[: n // 2].copy()
    b[:, :3] += rng.normal(scale=0.0003, size=(len(b), 3)).astype(np.float32)
    b = np.concatenate([b, obj[-n // 3:]])
    a[:, 6], a[:, 7] = rng.integers(1, 10, len(a)), 10
    b[:, 6], b[:, 7] = rng.integers(1, 30, len(b)), rng.integers(30, 41, len(b))
    return a, b


def test_the_constants():
    assert merge.COS_HALF_RAD.dtype == np.float32 and merge.COS_HALF_RAD == np.float32(math.cos(0.5))
    r = np.zeros((5, 12), np.float32)
    r[:, 11] = [0.004, np.nan, 0.002, np.inf, 0.003]
    assert merge.default_radius(r) == 2.0 * float(np.float32(0.003)) and merge.default_radius(r[:0]) == 0.0
    assert merge.default_radius(r[1:2]) == 0.0


def test_the_stamp_rewrite():
    a, b = maps()
    out = merge.rewrite_stamps(b, 10, 40)                           # B's clock is 30 ahead
    assert out is not b and np.array_equal(np.delete(out, [6, 7], 1), np.delete(b, [6, 7], 1))
    assert np.array_equal(out[:, 6:8], np.clip(b[:, 6:8] - 30, 1, 10)) and out[:, 6:8].min() == 1 and out[:, 6:8].max() == 10
    assert (b[:, 6] - 30 < 1).any()                                 # some stamps did fall before A's first frame
    later = merge.rewrite_stamps(b, 100, 40)                        # A is ahead: nothing lands in the future
    assert np.array_equal(later[:, 6:8], b[:, 6:8] + 60)
    bad = b.copy()
    bad[0, 6], bad[1, 7] = -5, 1e6
    assert merge.rewrite_stamps(bad, 50, 50)[0, 6] == 1 and merge.rewrite_stamps(bad, 50, 50)[1, 7] == 50
    with pytest.raises(ValueError):
        merge.rewrite_stamps(b, 0, 40)


def test_join_maps_on_the_restatement():
    a, b = maps()
    rec, stats, match, radius = merge.join_maps(a, b, None, 10, 40, merge=stand_in)
    assert radius == merge.default_radius(a) and sum(stats) == len(b) and len(rec) == len(a) + stats[2]
    assert stats[0] + stats[1] >= len(a) // 2 - 5 and stats[2] > 10 and len(match) == len(b)
    assert (rec[:, 6:8] >= 1).all() and (rec[:, 7] <= 10).all() and rec[:len(a), 6].tobytes() == a[:, 6].tobytes()
    again = merge.join_maps(a, b, np.eye(4), 10, 40, radius=radius, merge=stand_in)
    assert again[0].tobytes() == rec.tobytes() and again[3] == radius


def test_the_restatement_itself():
    a, _ = maps(257)
    a[:, 3] = 8.0
    rec, match, stats = mr.merge(a, a, None, 0.002, float(merge.COS_HALF_RAD))
    assert stats == [257, 0, 0, 0] and np.array_equal(match, np.arange(257)) and rec[:, :3].tobytes() == a[:, :3].tobytes() and (rec[:, 3] == 16).all()
    a2, b = maps()
    b[3, 0], b[4, 3], b[5, 11] = np.nan, 0.0, np.inf
    rec, match, stats = mr.merge(a2, b, rsn.motion(), 0.004, 0.0)
    assert sum(stats) == len(b) and stats[3] == 3 and (match[3:6] == -2).all()
    assert len(rec) == len(a2) + stats[2] and stats[2] == np.count_nonzero(match == -1) and stats[0] + stats[1] == np.count_nonzero(match >= 0)
    assert mr.merge(a2, b[:0], None, 0.004, 0.0)[0].tobytes() == a2.tobytes()
    assert mr.merge(a2[:0], b, None, 0.004, 0.0)[2] == [0, 0, len(b) - 3, 3]


# ---------------- the command ----------------
class FakeModel:
    def __init__(self, owner):
        self.o = owner

    def downloadMap(self):
        return self.o.map.copy()

    def lastCount(self):
        return len(self.o.map)

    def mergeMap(self, source, T=None, radius=None, min_cos=None):
        self.o.calls.append(dict(source=np.array(source), T=T, radius=radius, min_cos=min_cos))
        self.o.map, stats, _ = stand_in(self.o.map, source, T, radius, min_cos)
        return stats


class FakeMF:
    sessions = {}
    saved = {}

    def __init__(self, rec, tick):
        self.map, self.tick, self.calls, self.closed = rec, tick, [], False

    @classmethod
    def loadSession(cls, path):
        return cls(*cls.sessions[os.path.basename(path)])

    @staticmethod
    def sessionInfo(path):
        return {"user": b"blob"}

    def getTick(self):
        return self.tick

    def getBackgroundModel(self):
        return FakeModel(self)

    def saveSession(self, path, user=b""):
        FakeMF.saved[path] = (self.map.copy(), user, self.calls)

    def close(self):
        self.closed = True


def files(tmp_path, T=np.eye(4)):
    for n in ("A.mfs", "B.mfs"):
        (tmp_path / n).write_bytes(b"x")
    np.savetxt(str(tmp_path / "T.txt"), T, fmt="%.17g")
    return str(tmp_path / "A.mfs"), str(tmp_path / "B.mfs"), str(tmp_path / "T.txt")


def test_the_command_on_the_restatement(tmp_path, monkeypatch, capsys):
    from maskfusion_amd import api
    a, b = maps()
    T = rsn.motion()
    FakeMF.sessions = {"A.mfs": (a, 10), "B.mfs": (rsn.moved_records(b, np.linalg.inv(T)), 40)}
    monkeypatch.setattr(api, "MaskFusion", FakeMF)
    pa, pb, pt = files(tmp_path, T)
    out, ply = str(tmp_path / "m.mfs"), str(tmp_path / "m.ply")
    assert merge.main(["--a", pa, "--b", pb, "--init", pt, "-o", out, "--ply", ply, "--radius", "0.004", "--min-cos", "0.5"]) == 0
    line = json.loads(capsys.readouterr().out.strip())
    assert set(line) == {"averaged", "confidence_only", "appended", "dropped", "n_out", "radius", "inlier_share", "rmse"}
    rec, user, calls = FakeMF.saved[out]
    (call,) = calls
    assert user == b"blob" and call["radius"] == 0.004 and call["min_cos"] == 0.5 and np.array_equal(call["T"], np.loadtxt(pt))
    assert call["source"].tobytes() == merge.rewrite_stamps(FakeMF.sessions["B.mfs"][0], 10, 40).tobytes()
    assert line["averaged"] + line["confidence_only"] + line["appended"] + line["dropped"] == len(b) and line["n_out"] == len(rec) == len(a) + line["appended"]
    assert line["averaged"] > 50 and line["appended"] > 10 and line["radius"] == 0.004 and line["inlier_share"] is None
    from maskfusion_amd import eval as ev
    assert len(ev.read_ply(ply)) == len(rec)
    # --register-global: the transform comes from the registration, whose share and rmse are reported
    from maskfusion_amd import eval as ev2
    seen = []

    def fake_register(est, ref, voxel, **kw):
        seen.append((len(est), len(ref), voxel, sorted(kw)))
        return {"T": T, "inlier_share": 0.75, "rmse": 0.002}
    monkeypatch.setattr(ev2, "register_global", fake_register)
    assert merge.main(["--a", pa, "--b", pb, "--register-global", "0.02", "-o", out]) == 0
    line = json.loads(capsys.readouterr().out.strip())
    assert seen == [(len(b), len(a), 0.02, ["est_normals", "method", "ref_normals"])] and (line["inlier_share"], line["rmse"]) == (0.75, 0.002)
    assert line["radius"] == merge.default_radius(a) and FakeMF.saved[out][2][0]["min_cos"] == float(merge.COS_HALF_RAD)


@pytest.mark.parametrize("extra", [[], ["--init", "T", "--register-global", "0.02"], ["--register-global", "0"], ["--register-global", "nan"],
                                   ["--init", "T", "--radius", "0"], ["--init", "T", "--radius", "inf"], ["--init", "T", "--min-cos", "1.5"],
                                   ["--init", "T", "--min-cos", "nan"], ["--init", "missing.txt"], ["--init", "BAD"], ["--init", "T", "--a", "missing.mfs"]])
def test_the_command_refuses(tmp_path, capsys, extra):
    pa, pb, pt = files(tmp_path)
    bad = tmp_path / "bad.txt"
    bad.write_text("1 0 0 0\n0 2 0 0\n0 0 1 0\n0 0 0 1\n")              # not a rotation
    extra = [pt if x == "T" else str(bad) if x == "BAD" else x for x in extra]
    with pytest.raises(SystemExit) as e:
        merge.main(["--a", pa, "--b", pb, "-o", str(tmp_path / "o.mfs")] + extra)
    assert e.value.code == 2 and "merge" in capsys.readouterr().err
    assert not (tmp_path / "o.mfs").exists()


def test_the_driver_knows_the_flag():
    from maskfusion_amd import cli
    flags = cli.parse(["-redetectmerge", "-run"])
    assert "-redetectmerge" in flags and "-redetect" not in flags
