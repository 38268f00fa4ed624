"""-m gpu: the device label stage (mf_labels_gpu.hip, 16 kernels) held to the oracle pass by pass on inputs built to sit on its thresholds
and on the edges of its indexing (tests/label_cases.py), through mf_k_label_stage, which shows the stage's intermediates:
  A  component labels, count and statistics == connected_components4, at 3x3 (smallest legal), 7x40 (nine rows in a wavefront: the rowStart
     ballot), 63/64/65x5 (a row equal to a wavefront, one that straddles two), 257x9 (a 256-thread workgroup that straddles rows, P a multiple
     of neither 256 nor 1024), 1030x5 (a row longer than k_lab_relabel's workgroup); thirteen patterns each
  B  the labels after the five removeEdges sweeps == mfo_remove_edges at 32x8 (one tile), 37x13, 70x21 (partial tiles, the 5-pixel halo):
     areas 49 / 50 / 51, the five-pixel growth limit, neighbour order, a depth step one float either side of 0.008, the image border
  C  the votes and decisions == mf_segmentation_cpu: component size 160 / 161, the 65 % / 60 % / 5 % rules at and beside equality, the repaint
     box, class mismatch, the new-model rule and both its bounds, a projected id without a model, a dropped model, 256 masks x 64 models
  D  the closing for radius 0 ... 4 x iterations 1 ... 3 at 65x5 and 70x21
  E  the vote tables at their capacity (320x240 checkerboard, 38 401 components): 218 class ids fit, 219 are refused with MF_ESTATE
  F  150 fixed-seed random small images
Every case first asserts its reference-side preconditions on the oracle's output (tests/test_label_edges_host.py), then every output of the
stage -- labels, count, statistics, swept labels, label image, new-model decision, ignore map -- exactly: integer work, no tolerance.
tests/test_emu_label_edges.py runs this file on the CPU-executed kernels."""
import ctypes as C

import numpy as np
import pytest

import label_cases as lc
import test_label_edges_host as ref_side
from test_label_edges_host import CASES, NAMES, assert_output_equal, assert_preconditions, params11, reference, seg_params

pytestmark = pytest.mark.gpu

MF_ESTATE = -5


def run_stage(L, c, expect_rc=0):
    """the whole model list with its alive flags goes to the device; the oracle got the list without the dropped models"""
    P = c.W * c.H
    full, ign = np.zeros((c.H, c.W), np.uint8), np.zeros((c.H, c.W), np.uint8)
    has_new, new_cls, n_comp = C.c_int32(0), C.c_int32(-1), C.c_int32(-1)
    cid = np.ascontiguousarray(c.cls if len(c.cls) else [0], np.int32)
    mids, mc, alive = (np.ascontiguousarray(v, np.int32) for v in (c.model_ids, c.model_cls, c.alive))
    p = params11(seg_params(c))
    cap = P // 2 + 2
    lab_cc, lab_swept, stats = np.full((c.H, c.W), -7, np.int32), np.full((c.H, c.W), -7, np.int32), np.full((cap, 5), -7, np.int32)
    rc = L.mf_k_label_stage(c.W, c.H, c.binary.ctypes.data, c.depth.ctypes.data, c.mask.ctypes.data, cid.ctypes.data, len(c.cls), c.proj.ctypes.data,
                            mids.ctypes.data, mc.ctypes.data, len(c.model_ids), c.next_id, int(c.allow), p.ctypes.data, ign.ctypes.data, full.ctypes.data,
                            C.byref(has_new), C.byref(new_cls), alive.ctypes.data, lab_cc.ctypes.data, lab_swept.ctypes.data, stats.ctypes.data,
                            C.byref(n_comp), cap)
    assert rc == expect_rc, (c.name, rc)
    return dict(full=full, has_new=bool(has_new.value), new_class=new_cls.value, ignore=ign, cc=lab_cc, swept=lab_swept, stats=stats, n_comp=n_comp.value)


def assert_components_equal(c, got, ref):
    assert got["n_comp"] == ref["n_comp"], (c.name, "n_comp", got["n_comp"], ref["n_comp"])
    d = got["cc"] != ref["cc"]
    assert not d.any(), f"{c.name}: {int(d.sum())} component labels differ, first at (y, x) = {tuple(np.argwhere(d)[0])}"
    n = ref["n_comp"]
    bad = np.flatnonzero((got["stats"][1:n] != ref["stats"][1:n]).any(axis=1))
    assert not len(bad), f"{c.name}: statistics of {len(bad)} components differ, first {1 + bad[0]}: {got['stats'][1 + bad[0]]} != {ref['stats'][1 + bad[0]]}"


def assert_swept_equal(c, got, ref):
    d = got["swept"] != ref["swept"]
    assert not d.any(), f"{c.name}: {int(d.sum())} swept labels differ, first at (y, x) = {tuple(np.argwhere(d)[0])}"


def check(hip, name):
    c, ref = CASES[name], reference(name)
    assert_preconditions(c, ref)
    got = run_stage(hip, c)
    assert_components_equal(c, got, ref)
    assert_swept_equal(c, got, ref)
    assert_output_equal(c, got, ref)


@pytest.mark.parametrize("name", NAMES["A"])
def test_components_numbering_statistics(hip, oracle, name):
    check(hip, name)


@pytest.mark.parametrize("name", NAMES["B"])
def test_remove_edges_sweeps(hip, oracle, name):
    check(hip, name)


@pytest.mark.parametrize("name", NAMES["C"])
def test_votes_and_decisions(hip, oracle, name):
    check(hip, name)


@pytest.mark.parametrize("name", NAMES["D"])
def test_closing(hip, oracle, name):
    check(hip, name)


def test_vote_table_overflow_is_reported(hip, oracle):
    """38 401 components x 218 class ids = 8 371 418 entries fit the 8 388 608 of a vote table; x 219 do not: the call says so (MF_ESTATE)
    instead of voting into a truncated table, its component half stays readable, and the next call in the process is an ordinary one"""
    fits, after = lc.case_e(218), lc.case_e_after()
    assert 38401 * 218 <= (8 << 20) < 38401 * 219
    ref = ref_side.compute_reference(fits)
    assert_preconditions(fits, ref)
    got = run_stage(hip, fits)
    assert_components_equal(fits, got, ref)
    assert_swept_equal(fits, got, ref)
    assert_output_equal(fits, got, ref)
    over = lc.case_e(219)
    got = run_stage(hip, over, expect_rc=MF_ESTATE)
    assert_components_equal(over, got, ref)               # the same checkerboard, no person class: the same components
    assert not got["full"].any() and not got["ignore"].any() and not got["has_new"]     # nothing half-made comes back
    ref = ref_side.compute_reference(after)
    assert_preconditions(after, ref)
    got = run_stage(hip, after)
    assert_components_equal(after, got, ref)
    assert_swept_equal(after, got, ref)
    assert_output_equal(after, got, ref)


@pytest.mark.parametrize("name", NAMES["F"])
def test_random_sweep(hip, oracle, name):
    check(hip, name)
