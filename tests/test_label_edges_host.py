"""The host form of the label stage (mf_segmentation_labels, mf_labels.hip: the device stage's specification) on the crafted cases of
tests/label_cases.py that reach its output -- C (votes and decisions), D (the closing) and F (the fixed-seed random sweep) -- against the
oracle's restatement of MfSegmentation.cpp:220-522.  Integer / label work: every comparison is exact.  No GPU needed.

Also the reference side shared with tests/test_gpu_label_edges.py: reference() runs the oracle once per case (components, the swept labels
through mfo_remove_edges, the whole stage) and assert_preconditions() checks on THAT output what the case's builder says makes it bite,
before anyone looks at the product."""
import ctypes as C
import functools

import numpy as np
import pytest

import label_cases as lc

CASES = {c.name: c for c in lc.cases_a() + lc.cases_b() + lc.cases_c() + lc.cases_d() + [lc.random_case(s) for s in lc.F_SEEDS]}
NAMES = {k: [n for n in CASES if n.startswith(k + "-")] for k in "ABCDF"}


def seg_params(c):
    from oracle import mfo_mm
    return mfo_mm.default_seg_params(**c.seg)


def params11(prm):
    return np.array([prm.threshold, prm.weightDistance, prm.weightConvexity, prm.morphEdgeIterations, prm.morphEdgeRadius, prm.morphMaskIterations,
                     prm.morphMaskRadius, prm.removeEdges, prm.minRelSizeNew, prm.maxRelSizeNew, prm.personClassID], np.float32)


def live_models(c):
    """the model list after the jump rule's drop (entry 0, the background, never drops)"""
    keep = [i for i in range(len(c.model_ids)) if i == 0 or c.alive[i]]
    return [c.model_ids[i] for i in keep], [c.model_cls[i] for i in keep]


def compute_reference(c):
    from oracle import mfo_mm
    prm = seg_params(c)
    binary = c.binary.copy()
    if len(c.cls):       # MfSegmentation.cpp:221-235: person pixels leave the binary image before the components are found
        cls = np.asarray(c.cls)
        mid = np.where(c.mask < len(c.cls), c.mask, 0)
        binary[cls[mid] == prm.personClassID] = 0
    n, cc, stats = mfo_mm.connected_components4(binary)
    swept = mfo_mm.remove_edges(cc, stats, c.depth) if prm.removeEdges else cc.copy()
    ids, mcls = live_models(c)
    ign = np.zeros((c.H, c.W), np.uint8)
    full, has_new, new_cls = mfo_mm.mf_segmentation_cpu(c.W, c.H, c.binary, c.depth, c.mask, c.cls, c.proj, ids, mcls, c.next_id, c.allow, ign, prm)
    ref = dict(n_comp=n, cc=cc, stats=stats.copy(), swept=swept, full=full, has_new=has_new, new_class=new_cls, ignore=ign)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(name):
    return compute_reference(CASES[name])


def assert_preconditions(c, ref):
    pre, cc, swept, full = c.pre, ref["cc"], ref["swept"], ref["full"]
    if "n_comp" in pre:
        assert ref["n_comp"] == pre["n_comp"], (c.name, "n_comp", ref["n_comp"])
    if "n_comp_min" in pre:
        assert ref["n_comp"] >= pre["n_comp_min"], (c.name, "n_comp", ref["n_comp"])
    for (y, x), a in pre.get("area_at", []):
        assert cc[y, x] != 0 and ref["stats"][cc[y, x]][4] == a, (c.name, "area", (y, x), int(ref["stats"][cc[y, x]][4]))
    changed = int((swept != cc).sum())
    if "changed" in pre:
        assert changed == pre["changed"], (c.name, "changed", changed)
    if "changed_min" in pre:
        assert changed >= pre["changed_min"], (c.name, "changed", changed)
    for (y, x), src in pre.get("swept_at", []):
        if src is None:
            assert swept[y, x] == 0, (c.name, "swept", (y, x), int(swept[y, x]))
        else:
            assert cc[src] != 0 and swept[y, x] == cc[src], (c.name, "swept", (y, x), int(swept[y, x]), int(cc[src]))
    if pre.get("border_kept"):
        edge = np.ones((c.H, c.W), bool)
        edge[1:-1, 1:-1] = False
        assert np.array_equal(swept[edge], cc[edge]) and (swept[edge] == 0).all(), c.name
    if "depth_step" in pre:
        p, q, side = pre["depth_step"]
        d = float(np.abs(np.float32(c.depth[p] - c.depth[q])))        # fabsf of the float difference, widened to double
        assert (d < 0.008 and 0.008 - d < 1e-9) if side == "below" else (d > 0.008 and d - 0.008 < 1e-9), (c.name, d)
    for (y, x), v in pre.get("full_at", []):
        assert full[y, x] == v, (c.name, "full", (y, x), int(full[y, x]), v)
    for v in pre.get("full_has", []):
        assert (full == v).any(), (c.name, "full lacks", v)
    if "distinct_min" in pre:
        assert len(np.unique(full)) >= pre["distinct_min"], (c.name, len(np.unique(full)))
    if "ignore_min" in pre:
        assert int((ref["ignore"] != 0).sum()) >= pre["ignore_min"], (c.name, int((ref["ignore"] != 0).sum()))
    if "has_new" in pre:
        assert ref["has_new"] == pre["has_new"], (c.name, "has_new", ref["has_new"])
        if pre["has_new"]:
            assert (full == c.next_id).any(), (c.name, "next_id does not occur")
    if "new_class" in pre:
        assert ref["new_class"] == pre["new_class"], (c.name, "new_class", ref["new_class"])


def run_host(L, c):
    ids, mcls = live_models(c)
    full, ign = np.zeros((c.H, c.W), np.uint8), np.zeros((c.H, c.W), np.uint8)
    has_new, new_cls = C.c_int32(0), C.c_int32(-1)
    cid = np.ascontiguousarray(c.cls if len(c.cls) else [0], np.int32)
    mids, mc = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(mcls, np.int32)
    p = params11(seg_params(c))
    rc = L.mf_segmentation_labels(c.W, c.H, c.binary.ctypes.data, c.depth.ctypes.data, c.mask.ctypes.data, cid.ctypes.data, len(c.cls), c.proj.ctypes.data,
                                  mids.ctypes.data, mc.ctypes.data, len(ids), c.next_id, int(c.allow), p.ctypes.data, ign.ctypes.data, full.ctypes.data,
                                  C.byref(has_new), C.byref(new_cls))
    assert rc == 0, rc
    return dict(full=full, has_new=bool(has_new.value), new_class=new_cls.value, ignore=ign)


def assert_output_equal(c, got, ref):
    assert (got["has_new"], got["new_class"]) == (ref["has_new"], ref["new_class"]), (c.name, got["has_new"], got["new_class"], ref["has_new"], ref["new_class"])
    d = got["full"] != ref["full"]
    assert not d.any(), f"{c.name}: {int(d.sum())} pixels of the label image differ, first at (y, x) = {tuple(np.argwhere(d)[0])}"
    assert np.array_equal(got["ignore"], ref["ignore"]), f"{c.name}: ignore map differs"


@pytest.mark.parametrize("name", NAMES["C"] + NAMES["D"] + NAMES["F"])
def test_host_form_on_crafted_cases(oracle, name):
    from maskfusion_amd.lib import load
    c, ref = CASES[name], reference(name)
    assert_preconditions(c, ref)
    assert_output_equal(c, run_host(load(), c), ref)


def test_case_inventory():
    """every shape, pattern and threshold the builders promise is there: nothing was left out on the way"""
    assert len(NAMES["A"]) == len(lc.A_SHAPES) * len(lc.A_PATTERNS) == 91 and len(NAMES["B"]) == 21 and len(NAMES["C"]) == 19
    assert len(NAMES["D"]) == 30 and len(NAMES["F"]) == 150
    assert {(c.W, c.H) for n, c in CASES.items() if n.startswith("B-")} == {(32, 8), (37, 13), (70, 21)}
    ws = {CASES[n].W for n in NAMES["F"]}
    assert min(ws) == 3 and max(ws) >= 1030 and max(CASES[n].H for n in NAMES["F"]) == 40
    assert sum(1 for n in NAMES["F"] if 0 in CASES[n].alive[1:]) >= 10 and sum(1 for n in NAMES["F"] if len(CASES[n].cls)) >= 50
