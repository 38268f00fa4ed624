"""The host side of the view scores (maskfusion_amd.eval.view_metrics) on hand-made counters, and the numpy restatement of the device
definition (tests/view_restatement.py) on cases whose answer is known.  No GPU."""
import math

import numpy as np
import pytest

import view_restatement as vr
from maskfusion_amd import eval as ev

FIX = 1 << 24


def _row(pixels=0, covered=0, valid=0, pairs=0, within=0, l1=0.0, err=0, err_covered=0, ssim_pixels=0, ssim=0.0):
    return [pixels, covered, valid, pairs, within, round(l1 * FIX), err, err_covered, ssim_pixels, round(ssim * FIX)]


def _counts(rows):
    """(n_frames, n_groups, 10) uint64 from nested lists of Python ints (negative sums as two's complement)"""
    return np.array(rows, dtype=np.int64).view(np.uint64)


def test_every_formula():
    c = _counts([[_row(1000, 800, 900, 720, 540, l1=720 * 0.0125, err=3 * 1000 * 100, err_covered=3 * 800 * 25, ssim_pixels=600, ssim=600 * 0.75)]])
    m = ev.view_metrics(c)
    s = m["frames"][0][0]
    assert s["coverage"] == 0.8 and s["depth_coverage"] == 0.8 and s["depth_within_tau"] == 0.75
    assert s["depth_l1"] == pytest.approx(0.0125, abs=2.0 ** -24) and s["ssim"] == pytest.approx(0.75, abs=2.0 ** -24)
    assert s["psnr"] == pytest.approx(10 * math.log10(255 ** 2 / 100.0), rel=1e-12)          # a mean squared error of 100 per channel
    assert s["psnr_covered"] == pytest.approx(10 * math.log10(255 ** 2 / 25.0), rel=1e-12)
    g = m["groups"][0]
    assert g["group"] == 0 and g["pixels"] == 1000 and g["frames"] == 1
    assert {k: g[k] for k in ev.VIEW_KEYS} == s == g["mean"] and set(s) == set(ev.VIEW_KEYS)      # one frame: pooled = mean = the frame
    assert {k: m["summary"][k] for k in ev.VIEW_KEYS} == s and m["summary"]["frames"] == 1


def test_negative_ssim_sum_is_a_signed_counter():
    c = _counts([[_row(50, ssim_pixels=40, ssim=-40 * 0.25)]])
    assert c[0, 0, 9] > 1 << 63
    assert ev.view_metrics(c)["frames"][0][0]["ssim"] == -0.25


def test_zero_denominators_and_zero_errors_give_none():
    keys = set(ev.VIEW_KEYS)
    none_of = lambda row: {k for k, v in ev.view_metrics(_counts([[row]]))["frames"][0][0].items() if v is None}
    assert none_of(_row()) == keys                                                                  # an empty group: nothing is defined
    full = dict(pixels=10, covered=5, valid=6, pairs=4, within=1, l1=0.5, err=7, err_covered=3, ssim_pixels=2, ssim=1.0)
    assert none_of(_row(**full)) == set()
    assert none_of(_row(**dict(full, covered=0, pairs=0, within=0, l1=0, err_covered=0))) == {"depth_l1", "depth_within_tau", "psnr_covered"}
    assert none_of(_row(**dict(full, valid=0, pairs=0, within=0, l1=0))) == {"depth_coverage", "depth_l1", "depth_within_tau"}
    assert none_of(_row(**dict(full, pairs=0, within=0, l1=0))) == {"depth_l1", "depth_within_tau"}
    assert none_of(_row(**dict(full, ssim_pixels=0, ssim=0))) == {"ssim"}
    assert none_of(_row(**dict(full, err=0, err_covered=0))) == {"psnr", "psnr_covered"}            # identical images: no finite PSNR
    assert none_of(_row(**dict(full, err_covered=0))) == {"psnr_covered"}
    m = ev.view_metrics(_counts([[_row(**dict(full, covered=0, pairs=0, within=0, l1=0, err_covered=0))]]))
    assert m["frames"][0][0]["coverage"] == 0.0 and m["frames"][0][0]["depth_coverage"] == 0.0      # a zero numerator is a value


def test_pooled_against_the_mean_of_the_frames():
    """two frames of very different size: pooling weighs by pixels, the mean by frames; a frame where a score is undefined leaves the mean"""
    f0 = _row(1000, 1000, 1000, 1000, 1000, l1=1000 * 0.01, err=3000 * 4, err_covered=3000 * 4, ssim_pixels=500, ssim=500 * 0.9)
    f1 = _row(100, 20, 50, 10, 0, l1=10 * 0.11, err=300 * 400, err_covered=60 * 100, ssim_pixels=10, ssim=10 * 0.1)
    f2 = _row()                                                                                       # the group is not in the frame
    m = ev.view_metrics(_counts([[f0], [f1], [f2]]))
    g = m["groups"][0]
    assert g["frames"] == 2 and g["pixels"] == 1100
    assert g["coverage"] == 1020 / 1100 and g["mean"]["coverage"] == pytest.approx((1.0 + 0.2) / 2)
    assert g["depth_coverage"] == 1010 / 1050 and g["mean"]["depth_coverage"] == pytest.approx((1.0 + 0.2) / 2)
    assert g["depth_within_tau"] == 1000 / 1010 and g["mean"]["depth_within_tau"] == 0.5
    assert g["depth_l1"] == pytest.approx((10 + 1.1) / 1010, abs=1e-6) and g["mean"]["depth_l1"] == pytest.approx(0.06, abs=1e-6)
    assert g["ssim"] == pytest.approx((450 + 1) / 510, abs=1e-6) and g["mean"]["ssim"] == pytest.approx(0.5, abs=1e-6)
    psnr = lambda mse: 10 * math.log10(255 ** 2 / mse)
    assert g["psnr"] == pytest.approx(psnr((3000 * 4 + 300 * 400) / 3300.0)) and g["mean"]["psnr"] == pytest.approx((psnr(4) + psnr(400)) / 2)
    assert g["psnr_covered"] == pytest.approx(psnr((3000 * 4 + 60 * 100) / 3060.0)) and g["mean"]["psnr_covered"] == pytest.approx((psnr(4) + psnr(100)) / 2)
    assert all(v is None for v in m["frames"][2][0].values())


def test_groups_and_the_summary_over_them():
    a, b = _row(300, 300, 300, 300, 300, err=900, err_covered=900), _row(100, 0, 100, err=30000)
    m = ev.view_metrics(_counts([[a, b, _row()]]))
    assert [g["group"] for g in m["groups"]] == [0, 1, 2] and [g["pixels"] for g in m["groups"]] == [300, 100, 0]
    assert m["groups"][0]["coverage"] == 1.0 and m["groups"][1]["coverage"] == 0.0 and m["groups"][2]["coverage"] is None
    assert m["summary"]["coverage"] == 0.75 and m["summary"]["depth_coverage"] == 0.75              # all groups together
    assert m["summary"]["psnr"] == pytest.approx(10 * math.log10(255 ** 2 * 1200 / 30900.0))
    with pytest.raises(ValueError):
        ev.view_metrics(np.zeros((2, 10), np.uint64))


def test_sums_do_not_wrap():
    big = (1 << 62) + 12345
    m = ev.view_metrics(_counts([[_row(1 << 24, err=big, ssim_pixels=1)], [_row(1 << 24, err=big, ssim_pixels=1)]]))
    assert m["groups"][0]["psnr"] == pytest.approx(10 * math.log10(255.0 ** 2 * 3 * (1 << 25) / (2 * big)))


# ---------------------------------------------------------------- the restatement itself ----------------------------------------------------------------
def test_restatement_weights_and_known_answers():
    w = vr.weights()
    assert len(w) == 11 and w == w[::-1] and abs(sum(w) - 1.0) < 1e-15 and w[5] == max(w)
    assert w[5] / w[4] == pytest.approx(math.exp(1 / 4.5))                                          # sigma 1.5
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 250, (1, 13, 14, 3), dtype=np.uint8)
    r = np.concatenate([rgb, np.full((1, 13, 14, 1), 255, np.uint8)], -1)
    d = np.full((1, 13, 14), 2.0, np.float32)
    rd = d.copy()
    rd[0, 0, :7] = 0.0                  # holes
    rd[0, 1, :4] = 2.5                  # |dz| = 0.5
    d[0, 2, :3] = np.nan
    c = vr.counts(r, rd, rgb, d, None, 1, 3.0, 0.25)[0, 0].view(np.int64).tolist()
    assert c == [182, 175, 179, 172, 168, 4 * (FIX // 2), 0, 0, 3 * 4, 12 * FIX]                    # identical colours: SSIM exactly 1
    r[0, 6, 7, 1], r[0, 0, 0, 0] = rgb[0, 6, 7, 1] + 30, rgb[0, 0, 0, 0] + 1
    c = vr.counts(r, rd, rgb, d, None, 1, 3.0, 0.25)[0, 0].view(np.int64).tolist()
    assert c[6] == 901 and c[7] == 900 and 6 * FIX < c[9] < 12 * FIX                                # (0, 0) is a hole; (6, 7) lies in every window
    g = np.zeros((1, 13, 14), np.uint8)
    g[0, :, 7:] = 1
    g[0, 12, :] = 77
    two = vr.counts(r, rd, rgb, d, g, 2, 3.0, 0.25)[0].view(np.int64)
    assert two[:, 0].tolist() == [84, 84] and two[:, 8].tolist() == [6, 6] and two[:, 1].tolist() == [77, 84]


def test_abi_table_has_the_new_calls():
    """(tests/test_abi.py, unchanged, checks the header against the table; this only pins the two prototypes' lengths)"""
    from maskfusion_amd.lib import SYMBOLS
    assert len(SYMBOLS["mf_view_score_dev"][1]) == 13 and len(SYMBOLS["mf_sensor_render_view"][1]) == 2
