"""Crafted inputs for the label stage (MfSegmentation::performSegmentation, CPU half: components, the five removeEdges sweeps, the votes,
the 65 % / 60 % / 5 % rules, the new-model rule, the closing, the bounding-box repaint), each built to sit ON one threshold or one edge of
the device form's indexing.  Plain numpy: nothing here imports the product or the oracle, so a case is the same input for every
implementation that is held to it (tests/test_gpu_label_edges.py, tests/test_label_edges_host.py).

A Case is the argument list of the stage plus `pre`, the reference-side preconditions: what must hold in the ORACLE's output for the case to
bite (tests/test_label_edges_host.py: assert_preconditions).  A case that stops sitting on its threshold then fails loudly instead of passing
emptily.  Keys of `pre` ((y, x) pixel coordinates throughout):
  n_comp / n_comp_min  components including the background              area_at   [((y, x), area of the component there)]
  changed / changed_min  pixels the sweeps relabelled                    swept_at  [((y, x), (y2, x2) | None)] swept label there == the
  full_at  [((y, x), value of the final label image there)]                        component label at (y2, x2) (non-zero), or == 0
  full_has  values that occur in the final image   distinct_min  number of distinct values in it   ignore_min  pixels of the ignore map set
  has_new / new_class  the new-model decision       depth_step  ((y, x), (y2, x2), 'below' | 'above'): (double)|d1 - d2| against 0.008
  border_kept  the sweeps left the image's border pixels alone
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "W H binary depth mask cls proj model_ids model_cls alive next_id allow seg pre name")

FG = 255


def _case(name, binary, depth=None, mask=None, cls=(), proj=None, model_ids=(0,), model_cls=(-1,), alive=None, next_id=None, allow=True,
          seg=None, pre=None):
    H, W = binary.shape
    z8 = np.zeros((H, W), np.uint8)
    return Case(W, H, np.ascontiguousarray(binary, np.uint8), np.ascontiguousarray(np.full((H, W), 2.0) if depth is None else depth, np.float32),
                z8.copy() if mask is None else np.ascontiguousarray(mask, np.uint8), list(cls), z8.copy() if proj is None else np.ascontiguousarray(proj, np.uint8),
                list(model_ids), list(model_cls), [1] * len(model_ids) if alive is None else list(alive),
                int(max(model_ids) + 1) if next_id is None else next_id, bool(allow), dict(seg or {}), dict(pre or {}), name)


# ------------------------------------------------------------------------------------------------------------------------------------------
# A. components, numbering, statistics
# ------------------------------------------------------------------------------------------------------------------------------------------
A_SHAPES = [(3, 3), (7, 40), (63, 5), (64, 5), (65, 5), (257, 9), (1030, 5)]   # (W, H): see tests/test_gpu_label_edges.py for what each is for


def _all_fg(W, H):
    return np.full((H, W), FG, np.uint8), dict(n_comp=2, area_at=[((0, 0), W * H)])


def _all_bg(W, H):
    return np.zeros((H, W), np.uint8), dict(n_comp=1)


def _checker(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    b = np.where((xx + yy) % 2 == 0, FG, 0).astype(np.uint8)
    return b, dict(n_comp=1 + (W * H + 1) // 2)


def _serpentine(W, H):
    """full rows joined by one pixel at alternating ends: one component whose union chain runs through every row"""
    b = np.zeros((H, W), np.uint8)
    b[0::2, :] = FG
    for y in range(1, H, 2):
        b[y, W - 1 if (y // 2) % 2 == 0 else 0] = FG
    return b, dict(n_comp=2, area_at=[((0, 0), int((b != 0).sum()))])


def _spiral(W, H):
    """a one-pixel path wound inwards with one-pixel gaps: a cell is entered only if none of its other 4-neighbours is on the path"""
    b = np.zeros((H, W), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    b[0, 0] = FG

    def free(nx, ny, fx, fy):
        if not (0 <= nx < W and 0 <= ny < H) or b[ny, nx]:
            return False
        for ax, ay in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            qx, qy = nx + ax, ny + ay
            if (qx, qy) != (fx, fy) and 0 <= qx < W and 0 <= qy < H and b[qy, qx]:
                return False
        return True

    while True:
        if free(x + dx, y + dy, x, y):
            x, y = x + dx, y + dy
            b[y, x] = FG
            continue
        dx, dy = -dy, dx          # clockwise in image coordinates: right -> down -> left -> up
        if not free(x + dx, y + dy, x, y):
            break
    return b, dict(n_comp=2, area_at=[((0, 0), int((b != 0).sum()))])


def _u_shape(W, H):
    """a U whose right arm starts one row above the left one (the component's first raster pixel is on the right arm), a lone pixel before
    it in raster order and one inside it after"""
    b = np.zeros((H, W), np.uint8)
    b[0:, W - 1] = FG
    b[1:, 0] = FG
    b[H - 1, :] = FG
    n = 2
    pre_area = []
    if W >= 5:
        b[0, 2] = FG
        n += 1
        pre_area.append(((0, 2), 1))
        if H >= 5:
            b[2, 2] = FG
            n += 1
            pre_area.append(((2, 2), 1))
    pre_area.append(((0, W - 1), 2 * H - 1 + W - 2))
    return b, dict(n_comp=n, area_at=pre_area)


def _v_shape(W, H):
    """two-pixel-wide diagonal arms (4-connected staircases) that meet in the last row; the right arm starts a row above the left one"""
    b = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in (W - 1 - y, W - 2 - y):
            if 0 <= x < W:
                b[y, x] = FG
        if y >= 1:
            for x in (y - 1, y):
                if 0 <= x < W:
                    b[y, x] = FG
    lo, hi = min(H - 2, W - 1), max(W - 1 - H, 0)
    b[H - 1, min(lo, hi):max(lo, hi) + 1] = FG
    return b, dict(n_comp_min=2)


def _staircase(W, H):
    """diagonals three apart: 8-connected along each, never 4-connected"""
    yy, xx = np.mgrid[0:H, 0:W]
    b = np.where((xx - yy) % 3 == 0, FG, 0).astype(np.uint8)
    return b, dict(n_comp=1 + int((b != 0).sum()))


def _stripes(W, H):
    b = np.zeros((H, W), np.uint8)
    b[:, 0::2] = FG
    return b, dict(n_comp=1 + (W + 1) // 2, area_at=[((0, 0), H)])


def _run_pairs(W, H):
    """rows in threes: runs [16k+3, 16k+10] over runs [8k, 8k+5] over a blank row.  Each upper run starts in the middle of one lower run and
    ends in the middle of the next: overlaps whose first column is the upper run's start, and overlaps whose first column is the lower's"""
    b = np.zeros((H, W), np.uint8)
    upper = np.zeros(W, bool)
    lower = np.zeros(W, bool)
    for k in range(0, W, 8):
        lower[k:k + 6] = True
    for k in range(0, W, 16):            # every other upper run, so that upper runs do not touch each other
        upper[k + 3:k + 11] = True
    for y in range(0, H, 3):
        b[y, upper] = FG
        if y + 1 < H:
            b[y + 1, lower] = FG
    return b, dict(n_comp_min=2)


def _first_pixel(W, H):
    b = np.zeros((H, W), np.uint8)
    b[0, 0] = FG
    return b, dict(n_comp=2, area_at=[((0, 0), 1)])


def _last_pixel(W, H):
    b = np.zeros((H, W), np.uint8)
    b[H - 1, W - 1] = FG
    return b, dict(n_comp=2, area_at=[((H - 1, W - 1), 1)])


def _last_row_col(W, H):
    b = np.zeros((H, W), np.uint8)
    b[H - 1, :] = FG
    b[:, W - 1] = FG
    return b, dict(n_comp=2, area_at=[((H - 1, 0), W + H - 1)])


A_PATTERNS = [("all-fg", _all_fg), ("all-bg", _all_bg), ("checker", _checker), ("serpentine", _serpentine), ("spiral", _spiral), ("u", _u_shape),
              ("v", _v_shape), ("staircase", _staircase), ("stripes", _stripes), ("run-pairs", _run_pairs), ("first-pixel", _first_pixel),
              ("last-pixel", _last_pixel), ("last-row-col", _last_row_col)]


def cases_a():
    out = []
    for W, H in A_SHAPES:
        for pname, fn in A_PATTERNS:
            b, pre = fn(W, H)
            out.append(_case(f"A-{W}x{H}-{pname}", b, pre=pre))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# B. the removeEdges sweeps.  Designs are laid out in a 32x8 window (one tile of k_lab_sweep5) anchored at (ax, ay): (0, 0) in the 32x8 image;
# in the larger images an anchor that makes the window straddle the tile corner at (32, 8).  Outside the window everything is edge (0).
# ------------------------------------------------------------------------------------------------------------------------------------------
B_SHAPES = [(32, 8, 0, 0), (37, 13, 5, 4), (70, 21, 20, 4)]   # W, H, ax, ay


def _b_absorbers(W, H, ax, ay):
    b = np.zeros((H, W), np.uint8)
    b[ay:ay + 5, ax:ax + 10] = FG                         # 50: absorbs nothing (a neighbour needs MORE than 50)
    b[ay:ay + 5, ax + 16:ax + 26] = FG
    b[ay + 5, ax + 16] = FG                               # 51: absorbs the edge pixels around it, five deep
    y = ay + 2
    return b, dict(n_comp=3, area_at=[((ay, ax), 50), ((ay, ax + 16), 51)], changed_min=5 * 3,
                   swept_at=[((y, ax + 11), (ay, ax + 16)), ((y, ax + 15), (ay, ax + 16)), ((y, ax + 10), None), ((ay + 5, ax + 3), None),
                             ((ay + 6, ax + 16), (ay, ax + 16))])


def _b_absorbed(W, H, ax, ay):
    b = np.zeros((H, W), np.uint8)
    b[ay:ay + 7, ax:ax + 7] = FG                          # 49: eaten from the side of the large component
    b[ay:ay + 8, ax + 8:ax + 16] = FG                     # 64
    b[ay:ay + 7, ax + 17:ax + 24] = FG
    b[ay + 7, ax + 17] = FG                               # 50: stays (a component is eaten only BELOW 50)
    y = ay + 3
    return b, dict(n_comp=4, area_at=[((ay, ax), 49), ((ay, ax + 8), 64), ((ay, ax + 17), 50)], changed_min=10,
                   swept_at=[((y, ax + 7), (ay, ax + 8)), ((y, ax + 6), (ay, ax + 8)), ((y, ax + 3), (ay, ax + 8)), ((y, ax + 2), (ay, ax)),
                             ((y, ax + 16), (ay, ax + 8)), ((y, ax + 17), (ay, ax + 17)), ((y, ax + 20), (ay, ax + 17))])


def _b_growth(W, H, ax, ay):
    """a 12-pixel edge band over the full height between two large components; in the larger images it holds the tile boundary x = 32"""
    x0 = {32: 10, 37: 21, 70: 26}[W]
    b = np.full((H, W), FG, np.uint8)
    b[:, x0:x0 + 12] = 0
    sw = [((y, x0 + k), (0, 0)) for y in (1, H // 2, H - 2) for k in range(5)]
    sw += [((y, x0 + 7 + k), (0, W - 1)) for y in (1, H // 2, H - 2) for k in range(5)]
    sw += [((y, x0 + k), None) for y in (1, H // 2, H - 2) for k in (5, 6)]
    sw += [((0, x0 + k), None) for k in range(12)] + [((H - 1, x0 + k), None) for k in range(12)]
    return b, dict(n_comp=3, changed=10 * (H - 2), swept_at=sw)


def _b_order(W, H, ax, ay):
    """one-pixel edge lines between a component above and two below: every edge pixel sees two or three components and takes the first in
    row-major neighbour order"""
    hT, xs = H // 2 - 1, W // 2 - 1
    b = np.full((H, W), FG, np.uint8)
    b[hT, :] = 0
    b[hT:, xs] = 0
    return b, dict(n_comp=4, changed=(W - 2) + (H - 2 - hT),
                   swept_at=[((hT, 1), (0, 0)), ((hT, xs), (0, 0)), ((hT, W - 2), (0, 0)), ((hT + 1, xs), (hT + 1, 0)), ((H - 2, xs), (hT + 1, 0)),
                             ((hT, 0), None), ((H - 1, xs), None)])


def depth_pair(which):
    """(a, b): float32 depths with a - b exact in float32 and, widened to double, just above 0.008 (a - b == 0.008f, the float nearest 0.008,
    which is LARGER than the double 0.008) or just below (the float before it).  Depths near 2 m cannot do this -- their differences are
    multiples of 2^-22 -- so the pair sits where the spacing of floats is 2^-30 or finer."""
    step = np.float32(0.008) if which == "above" else np.nextafter(np.float32(0.008), np.float32(0))
    b = np.float32(5368709 * 2.0 ** -30)       # ~0.005, a multiple of 2^-30
    a = np.float32(b + step)
    assert np.float32(a - b) == step and float(a) - float(b) == float(step)     # the subtraction is exact
    assert (float(step) > 0.008) if which == "above" else (float(step) < 0.008)
    return a, b


def _b_depth(which):
    def build(W, H, ax, ay):
        a, d0 = depth_pair(which)
        b = np.full((H, W), FG, np.uint8)
        b[:, W // 2:] = 0                       # component on the left at depth d0, edge pixels on the right at depth a
        depth = np.full((H, W), d0, np.float32)
        depth[:, W // 2:] = a
        x = W // 2
        if which == "below":
            pre = dict(n_comp=2, changed=5 * (H - 2), depth_step=((1, x), (1, x - 1), "below"),
                       swept_at=[((1, x), (0, 0)), ((H - 2, x + 4), (0, 0)), ((1, x + 5), None)])
        else:
            pre = dict(n_comp=2, changed=0, depth_step=((1, x), (1, x - 1), "above"), swept_at=[((1, x), None)])
        return b, pre, depth
    return build


def _b_border(W, H, ax, ay):
    """a component two pixels inside the image: the ring next to it fills, the image's own border ring never changes"""
    b = np.zeros((H, W), np.uint8)
    b[2:H - 2, 2:W - 2] = FG
    return b, dict(n_comp=2, changed=2 * (W - 2) + 2 * (H - 4), border_kept=True,
                   swept_at=[((1, 1), (2, 2)), ((H - 2, W - 2), (2, 2)), ((0, 0), None), ((0, W // 2), None), ((H - 1, W - 1), None), ((H // 2, 0), None),
                             ((H // 2, W - 1), None)])


B_DESIGNS = [("absorbers", _b_absorbers), ("absorbed", _b_absorbed), ("growth", _b_growth), ("order", _b_order), ("depth-below", _b_depth("below")),
             ("depth-above", _b_depth("above")), ("border", _b_border)]


def cases_b():
    out = []
    for W, H, ax, ay in B_SHAPES:
        for dname, fn in B_DESIGNS:
            r = fn(W, H, ax, ay)
            out.append(_case(f"B-{W}x{H}-{dname}", r[0], depth=r[2] if len(r) > 2 else None, pre=r[1]))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# C. votes and decisions (64x40 unless stated; P = 2560)
# ------------------------------------------------------------------------------------------------------------------------------------------
CW, CH = 64, 40
_CRISP = dict(morphMaskIterations=0, removeEdges=0)     # nothing between the votes and the output


def _blank(W=CW, H=CH):
    return np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)


def _c_component_size():
    b, m, p = _blank()
    b[2:12, 2:18] = FG                                   # 160: not mapped (needs MORE than minMappedComponentSize)
    b[2:12, 30:46] = FG; b[12, 30] = FG                  # 161
    m[b != 0] = 1
    return _case("C-component-size", b, mask=m, cls=[0, 41], seg=dict(_CRISP, minRelSizeNew=0.01), next_id=1,
                 pre=dict(n_comp=3, area_at=[((2, 2), 160), ((2, 30), 161)], full_at=[((5, 5), 0), ((5, 35), 1), ((12, 30), 1)], has_new=True, new_class=41))


def _c_65_percent():
    b, m, p = _blank()
    b[2:12, 2:22] = FG; m[2:12, 2:15] = 1                                    # 200 with 130 mask pixels: (int)(0.65f * 200) == 130, not mapped
    b[2:12, 30:50] = FG; m[2:12, 30:43] = 1; m[2, 43] = 1                    # 200 with 131
    assert int(np.float32(0.65) * np.float32(200)) == 130
    return _case("C-65-percent", b, mask=m, cls=[0, 41], seg=dict(_CRISP, minRelSizeNew=0.01), next_id=1,
                 pre=dict(n_comp=3, area_at=[((2, 2), 200), ((2, 30), 200)], full_at=[((5, 5), 0), ((5, 20), 0), ((5, 35), 1), ((5, 48), 1)], has_new=True))


def _c_65_percent_float():
    """the threshold is a FLOAT product: 0.65f * 180 rounds to the float below 117, so (int) gives 116 where the exact product gives 117.
    A 180-pixel component with 117 mask pixels is mapped, one with 116 is not"""
    b, m, p = _blank()
    assert int(np.float32(0.65) * np.float32(180)) == 116 and int(0.65 * 180) == 117
    b[2:12, 2:20] = FG; m[2:8, 2:20] = 1; m[8, 2:10] = 1                     # 180 with 116
    b[2:12, 30:48] = FG; m[2:8, 30:48] = 1; m[8, 30:39] = 1                  # 180 with 117
    return _case("C-65-percent-float", b, mask=m, cls=[0, 41], seg=dict(_CRISP, minRelSizeNew=0.01), next_id=1,
                 pre=dict(n_comp=3, area_at=[((2, 2), 180), ((2, 30), 180)], full_at=[((5, 5), 0), ((5, 35), 1), ((11, 47), 1)], has_new=True))


def _c_60_percent():
    b, m, p = _blank()
    b[2:12, 2:22] = FG; p[2:8, 2:22] = 3                                     # 200, model overlap 120: stays 0
    b[2:12, 30:50] = FG; p[2:8, 30:50] = 3; p[8, 30] = 3                     # 200, overlap 121: follows model 3
    assert not np.float32(120) > np.float32(0.6) * np.float32(200) and np.float32(121) > np.float32(0.6) * np.float32(200)
    return _case("C-60-percent", b, proj=p, model_ids=[0, 3], model_cls=[-1, 41], seg=_CRISP,
                 pre=dict(n_comp=3, full_at=[((5, 5), 0), ((10, 5), 0), ((5, 35), 3), ((11, 49), 3)], has_new=False))


def _c_60_percent_equal():
    """0.6f * 160 rounds to 96 exactly in float32: an overlap of 96 is NOT more than 60 % (the 200-pixel pair cannot tell > from >=, since
    0.6f * 200 rounds to the float above 120), 97 is"""
    b, m, p = _blank()
    assert np.float32(0.6) * np.float32(160) == np.float32(96)
    b[2:12, 2:18] = FG; p[2:8, 2:18] = 3                                     # 160, overlap 96
    b[2:12, 30:46] = FG; p[2:8, 30:46] = 3; p[8, 30] = 3                     # 160, overlap 97
    return _case("C-60-percent-equal", b, proj=p, model_ids=[0, 3], model_cls=[-1, 41], seg=_CRISP,
                 pre=dict(n_comp=3, area_at=[((2, 2), 160), ((2, 30), 160)], full_at=[((5, 5), 0), ((5, 35), 3)]))


def _c_repaint_box():
    """no masks, model 1 projects everywhere, flat depth: both components grow five pixels into the edge around them and follow model 1, but
    only the pre-sweep box plus one column and one row is repainted"""
    b, m, p = _blank()
    b[4:14, 4:24] = FG                                   # box x 4..23, y 4..13 -> repainted x 4..24, y 4..14; swept to x 1..28, y 1..18
    b[30:40, 50:64] = FG                                 # touches the last column and the last row: the box is clamped
    p[:] = 1
    return _case("C-repaint-box", b, proj=p, model_ids=[0, 1], model_cls=[-1, 41], seg=dict(morphMaskIterations=0),
                 pre=dict(n_comp=3, changed_min=300,
                          swept_at=[((15, 25), (4, 4)), ((18, 28), (4, 4)), ((14, 26), (4, 4)), ((16, 24), (4, 4)), ((3, 3), (4, 4)), ((25, 45), (30, 50))],
                          full_at=[((4, 4), 1), ((14, 24), 1), ((14, 4), 1), ((4, 24), 1), ((14, 25), 0), ((15, 24), 0), ((15, 25), 0), ((3, 4), 0), ((4, 3), 0),
                                   ((39, 63), 1), ((30, 50), 1), ((29, 50), 0), ((30, 49), 0), ((38, 62), 1)]))


def _c_5_percent(k):
    """mask 1 holds two 200-pixel components (maskPixels 400; 0.05f * 400 == 20 exactly in float32); model 1 of the mask's class overlaps it
    on k pixels: under 20 the mask spawns a new model, at 20 (not LESS than 5 %) and over it keeps model 1"""
    def build():
        b, m, p = _blank()
        assert np.float32(0.05) * np.float32(400) == np.float32(20)
        b[2:12, 2:22] = FG; b[2:12, 30:50] = FG
        m[b != 0] = 1
        p.reshape(-1)[np.flatnonzero(b.reshape(-1))[:k]] = 1
        want = 2 if k < 20 else 1
        return _case(f"C-5-percent-{k}", b, mask=m, cls=[0, 41], proj=p, model_ids=[0, 1], model_cls=[-1, 41], next_id=2, seg=dict(_CRISP, minRelSizeNew=0.01),
                     pre=dict(n_comp=3, full_at=[((5, 5), want), ((5, 35), want)], has_new=k < 20))
    return build


def _c_class_mismatch():
    b, m, p = _blank()
    b[2:12, 2:22] = FG; m[2:12, 2:22] = 1; p[2:12, 2:22] = 1
    b[20:30, 2:22] = FG; m[20:30, 2:22] = 2; p[20:30, 2:22] = 2
    return _case("C-class-mismatch", b, mask=m, cls=[0, 41, 42], proj=p, model_ids=[0, 1, 2], model_cls=[-1, 99, 42], next_id=3, seg=dict(_CRISP, minRelSizeNew=0.01),
                 pre=dict(n_comp=3, full_at=[((5, 5), 255), ((25, 5), 2)], has_new=False))


def _c_two_new():
    b, m, p = _blank()
    b[2:12, 2:22] = FG; m[2:12, 2:22] = 1
    b[20:30, 2:22] = FG; m[20:30, 2:22] = 2
    return _case("C-two-new", b, mask=m, cls=[0, 41, 42], next_id=1, seg=dict(_CRISP, minRelSizeNew=0.01),
                 pre=dict(n_comp=3, full_at=[((5, 5), 1), ((25, 5), 255)], has_new=True, new_class=41))


def _c_rel_size(which, area, spawns):
    """one component of `area` pixels wholly under mask 1: maskPixels == area, against (size_t)(0.07f * 2560) == 179 and (size_t)(0.4f * 2560) == 1024"""
    def build():
        b, m, p = _blank()
        assert int(np.float32(0.07) * np.float32(CW * CH)) == 179 and int(np.float32(0.4) * np.float32(CW * CH)) == 1024
        rows, rest = divmod(area, 32)
        b[2:2 + rows, 2:34] = FG
        b[2 + rows, 2:2 + rest] = FG
        assert int((b != 0).sum()) == area
        m[b != 0] = 1
        return _case(f"C-{which}-{area}", b, mask=m, cls=[0, 41], next_id=1, seg=_CRISP,
                     pre=dict(n_comp=2, area_at=[((2, 2), area)], full_at=[((2, 2), 1 if spawns else 255)], has_new=spawns, new_class=41 if spawns else -1))
    return build


def _c_projected_without_model():
    """projected id 7 has no model: in the component table its pixels vote for the background (index 0, the std::map default), in the mask
    table they have no row"""
    b, m, p = _blank()
    b[2:12, 2:22] = FG; p[2:12, 2:17] = 7; p[2:12, 17:22] = 1             # 150 votes for the background, 50 for model 1: follows nothing
    b[20:30, 2:22] = FG; p[20:26, 2:22] = 1; p[26:30, 2:22] = 7           # 120 + 80: 120 is not more than 60 %
    b[2:12, 30:50] = FG; m[2:12, 30:50] = 1; p[2:12, 30:50] = 7           # mask 1 overlaps no model: spawns
    b[20:30, 30:50] = FG; p[20:30, 30:50] = 1; p[20:23, 30:50] = 7        # 140 for model 1: follows it
    return _case("C-projected-without-model", b, mask=m, cls=[0, 41], proj=p, model_ids=[0, 1], model_cls=[-1, 41], next_id=2, seg=dict(_CRISP, minRelSizeNew=0.01),
                 pre=dict(n_comp=5, full_at=[((5, 5), 0), ((5, 20), 0), ((22, 5), 0), ((5, 35), 2), ((25, 35), 1), ((20, 30), 1)], has_new=True))


def _c_dropped_model():
    """models 2, 4, 5 with 4 dropped by the jump rule: what 4 projects votes for the background, model 5 moves up one index"""
    b, m, p = _blank()
    b[2:12, 2:22] = FG; p[2:12, 2:22] = 4                                  # would follow 4
    b[20:30, 2:22] = FG; p[20:30, 2:22] = 5
    b[2:12, 30:50] = FG; p[2:12, 30:50] = 2
    b[20:30, 30:50] = FG; m[20:30, 30:50] = 1; p[20:30, 30:50] = 4        # mask 1 of model 4's class: spawns instead
    b[32:38, 2:42] = FG; m[32:38, 2:42] = 2; p[32:38, 2:42] = 5           # mask 2 keeps model 5
    return _case("C-dropped-model", b, mask=m, cls=[0, 44, 45], proj=p, model_ids=[0, 2, 4, 5], model_cls=[-1, 42, 44, 45], alive=[1, 1, 0, 1], next_id=6,
                 seg=dict(_CRISP, minRelSizeNew=0.01),
                 pre=dict(n_comp=6, full_at=[((5, 5), 0), ((25, 5), 5), ((5, 35), 2), ((25, 35), 6), ((35, 5), 5)], has_new=True, new_class=44))


def _c_person():
    """a person-class mask cuts its pixels out of the components and sets the ignore map"""
    b, m, p = _blank()
    b[2:22, 2:42] = FG
    m[2:22, 2:20] = 1
    m[2:22, 21:23] = 2                                   # person: splits the component in two
    return _case("C-person", b, mask=m, cls=[0, 41, 255], next_id=1, seg=dict(morphMaskIterations=1, minRelSizeNew=0.01),
                 pre=dict(n_comp=3, ignore_min=40, full_at=[((5, 21), 255), ((5, 5), 1), ((5, 30), 0)], has_new=True))


def _c_many():
    """256 x 64: 64 cells of 16 x 16, each a 14 x 14 component (196) mostly under its own mask value; every mask value 0 ... 255 occurs;
    64 models, model j projecting over cell j: matching classes, mismatching classes, one person class, one cell without a model"""
    W, H = 256, 64
    b, m, p = _blank(W, H)
    cls = [0] + [40 + (k % 7) for k in range(1, 256)]
    model_ids, model_cls = [0], [-1]
    for c in range(64):
        cx, cy = (c % 16) * 16, (c // 16) * 16
        b[cy + 1:cy + 15, cx + 1:cx + 15] = FG
        vals = [(4 * c + 1 + k) % 256 for k in range(4)]
        m[cy + 1:cy + 15, cx + 1:cx + 15] = vals[0]
        m[cy + 1:cy + 4, cx + 1:cx + 15] = vals[1]      # 42 of 196 under the next value: 154 stay, more than (int)(0.65f * 196) == 127
        m[cy, cx:cx + 16] = vals[2]
        m[cy + 15, cx:cx + 16] = vals[3]
        if c >= 1:
            model_ids.append(c)
            model_cls.append(cls[vals[0]] if c % 3 else 99)          # every third model has another class than its mask
            p[cy + 1:cy + 15, cx + 1:cx + 9] = c
    cls[4 * 20 + 1] = 255                                             # cell 20's mask is a person
    assert int(np.float32(0.65) * np.float32(196)) == 127 and len(np.unique(m)) == 256
    return _case("C-many-256x64", b, mask=m, cls=cls, proj=p, model_ids=model_ids, model_cls=model_cls, next_id=64,
                 seg=dict(morphMaskIterations=1, minRelSizeNew=0.005),
                 pre=dict(n_comp_min=64, has_new=True, distinct_min=40, full_has=[0, 1, 2, 64, 255], ignore_min=150))


C_BUILDERS = [_c_component_size, _c_65_percent, _c_65_percent_float, _c_60_percent, _c_60_percent_equal, _c_repaint_box, _c_5_percent(19), _c_5_percent(20), _c_5_percent(21),
              _c_class_mismatch, _c_two_new, _c_rel_size("min-rel-size", 179, False), _c_rel_size("min-rel-size", 180, True),
              _c_rel_size("max-rel-size", 1023, True), _c_rel_size("max-rel-size", 1024, False), _c_projected_without_model, _c_dropped_model,
              _c_person, _c_many]


def cases_c():
    return [f() for f in C_BUILDERS]


# ------------------------------------------------------------------------------------------------------------------------------------------
# D. the closing of the label image: blobs of different values one and two pixels apart and against every border
# ------------------------------------------------------------------------------------------------------------------------------------------
def _d_narrow(r, it):
    """65 x 5 holds one component large enough to be mapped (34 x 5 = 170): its label meets the ignore value 255 (person patches), which wins
    every dilation, at gaps of one and two pixels, a one-pixel hole, and patches on and near the right border"""
    W, H = 65, 5
    b, m, p = _blank(W, H)
    b[:, 1:35] = FG                                       # one pixel from the left border, on the top and bottom ones
    b[2, 10] = 0                                          # a hole of one edge pixel
    m[:, 1:35] = 1
    m[0:2, 36:40] = 2                                     # person, one pixel from the component
    m[3:5, 37:41] = 2                                     # person, two pixels from it
    m[2, 62:65] = 2                                       # on the right border
    m[0, 58:60] = 2
    m[4, 20] = 2                                          # inside the component, on the bottom border
    return _case(f"D-65x5-r{r}-i{it}", b, mask=m, cls=[0, 41, 255], next_id=1,
                 seg=dict(removeEdges=0, morphMaskRadius=r, morphMaskIterations=it, minRelSizeNew=0.01, maxRelSizeNew=0.9),
                 pre=dict(n_comp=2, has_new=True, full_has=[1, 255], full_at=[((0, 1), 1), ((2, 63), 255)], ignore_min=20))


def _d_wide(r, it):
    """70 x 21: six mapped components, each under its own mask and kept by its own model (label = 10 + mask value), one and two pixels apart
    and on every border; a person patch between them"""
    W, H = 70, 21
    b, m, p = _blank(W, H)
    boxes = [(0, 14, 0, 12), (0, 14, 13, 25), (0, 14, 27, 39), (7, 21, 58, 70), (15, 21, 0, 28), (15, 21, 29, 57)]   # y0, y1, x0, x1
    cls, ids, mcls = [0], [0], [-1]
    for k, (y0, y1, x0, x1) in enumerate(boxes, 1):
        b[y0:y1, x0:x1] = FG
        m[y0:y1, x0:x1] = k
        p[y0:y1, x0:x1] = 10 + k
        cls.append(40 + k); ids.append(10 + k); mcls.append(40 + k)
    cls.append(255)
    m[0:5, 41:44] = 7                                     # person patch, two pixels from the third component, on the top border
    m[2:4, 68:70] = 7                                     # ... and one on the right border above the fourth
    return _case(f"D-70x21-r{r}-i{it}", b, mask=m, cls=cls, proj=p, model_ids=ids, model_cls=mcls, next_id=20,
                 seg=dict(removeEdges=0, morphMaskRadius=r, morphMaskIterations=it),
                 pre=dict(n_comp=7, has_new=False, full_has=[11, 12, 13, 14, 15, 16, 255],
                          full_at=[((1, 1), 11), ((1, 14), 12), ((1, 28), 13), ((20, 69), 14), ((20, 0), 15), ((20, 40), 16), ((1, 42), 255)]))


def cases_d():
    return [f(r, it) for f in (_d_narrow, _d_wide) for r in range(0, 5) for it in range(1, 4)]


# ------------------------------------------------------------------------------------------------------------------------------------------
# E. vote tables at their capacity: 320 x 240 checkerboard, 38 401 components
# ------------------------------------------------------------------------------------------------------------------------------------------
def case_e(n_class_ids):
    W, H = 320, 240
    yy, xx = np.mgrid[0:H, 0:W]
    b = np.where((xx + yy) % 2 == 0, FG, 0).astype(np.uint8)
    rng = np.random.default_rng(219)
    m = rng.integers(0, n_class_ids, (H, W)).astype(np.uint8)
    cls = [0] + [41 + (k % 5) for k in range(1, n_class_ids)]
    return _case(f"E-checker-{n_class_ids}", b, mask=m, cls=cls, next_id=1, seg=dict(morphMaskIterations=1), pre=dict(n_comp=38401, has_new=False))


def case_e_after():
    """an ordinary frame for the call that follows the refused one"""
    W, H = 320, 240
    b = np.full((H, W), FG, np.uint8)
    b[::40, :] = 0; b[:, ::64] = 0
    m = np.zeros((H, W), np.uint8)
    m[41:80, 65:128] = 1
    m[121:160, 129:192] = 2
    p = np.zeros((H, W), np.uint8)
    p[121:160, 129:192] = 1
    return _case("E-after", b, mask=m, cls=[0, 41, 42], proj=p, model_ids=[0, 1], model_cls=[-1, 42], next_id=2, seg=dict(minRelSizeNew=0.01),
                 pre=dict(n_comp_min=20, has_new=True, new_class=41, full_has=[0, 1, 2]))


# ------------------------------------------------------------------------------------------------------------------------------------------
# F. fixed-seed random sweep: blocky binaries, depth in 4 mm steps (so that neighbours differ by 0, 4, 8 or 12 mm), random masks, models,
# dropped models, parameters; widths 3 ... 1030, heights 3 ... 40
# ------------------------------------------------------------------------------------------------------------------------------------------
F_WIDTHS = [3, 4, 5, 7, 16, 31, 32, 33, 37, 63, 64, 65, 70, 100, 127, 128, 129, 200, 255, 256, 257, 320, 511, 512, 513, 640, 1023, 1024, 1025, 1030]
F_HEIGHTS = [3, 4, 5, 7, 8, 9, 13, 16, 17, 21, 32, 40]
F_SEEDS = list(range(150))


def _blocks(rng, W, H, n, vmax):
    img = np.zeros((H, W), np.uint8)
    for _ in range(n):
        w, h = int(rng.integers(1, max(2, W // 2 + 1))), int(rng.integers(1, max(2, H // 2 + 1)))
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        img[y:y + h, x:x + w] = int(rng.integers(1, vmax + 1))
    return img


def random_case(seed):
    rng = np.random.default_rng(7000 + seed)
    W, H = int(rng.choice(F_WIDTHS)), int(rng.choice(F_HEIGHTS))
    # blocky binary: cells of a random pitch switched on or off, then random edge lines and speckle
    pitch = int(rng.choice([1, 2, 3, 5, 8, 13]))
    cells = rng.random(((H + pitch - 1) // pitch, (W + pitch - 1) // pitch)) < rng.choice([0.5, 0.75, 0.9, 1.0])
    b = np.kron(cells.astype(np.uint8), np.ones((pitch, pitch), np.uint8))[:H, :W].astype(bool)
    for _ in range(int(rng.integers(0, 6))):
        if rng.integers(0, 2):
            b[int(rng.integers(0, H)), :] = False
        else:
            b[:, int(rng.integers(0, W))] = False
    b &= rng.random((H, W)) >= rng.choice([0.0, 0.01, 0.05])
    binary = np.where(b, FG, 0).astype(np.uint8)
    steps = np.kron(rng.integers(0, 4, ((H + 3) // 4, (W + 6) // 7)), np.ones((4, 7), np.int64))[:H, :W]
    depth = (np.float32(1.5) + np.float32(0.004) * steps.astype(np.float32)).astype(np.float32)
    depth[rng.random((H, W)) < 0.03] = 0.0
    n_masks = int(rng.choice([0, 0, 2, 3, 5, 9]))
    mask = _blocks(rng, W, H, int(rng.integers(1, 8)), n_masks - 1) if n_masks > 1 else np.zeros((H, W), np.uint8)
    if n_masks and rng.integers(0, 4) == 0:
        mask[int(rng.integers(0, H)), :] = 255              # values without a class id count as "no mask"
    cls = ([0] + [int(rng.choice([41, 42, 56, 255])) for _ in range(n_masks - 1)]) if n_masks else []
    n_models = int(rng.integers(1, 6))
    ids = [0] + sorted(rng.choice(np.arange(1, 12), n_models - 1, replace=False).tolist())
    mcls = [-1] + [int(rng.choice([41, 42, 56])) for _ in range(n_models - 1)]
    alive = [1] + [int(rng.random() < 0.8) for _ in range(n_models - 1)]
    pb = _blocks(rng, W, H, int(rng.integers(0, 6)), 12)
    proj = np.where(np.isin(pb, ids + [12]), pb, 0).astype(np.uint8)     # 12: a projected id without a model
    seg = dict(morphMaskIterations=int(rng.integers(0, 3)), morphMaskRadius=int(rng.integers(0, 4)), removeEdges=int(rng.integers(0, 4) > 0),
               minRelSizeNew=float(rng.choice([0.004, 0.02, 0.07])), maxRelSizeNew=float(rng.choice([0.4, 0.9])))
    return _case(f"F-{seed}-{W}x{H}", binary, depth=depth, mask=mask, cls=cls, proj=proj, model_ids=ids, model_cls=mcls, alive=alive,
                 next_id=int(max(ids) + 1), allow=bool(rng.integers(0, 4) > 0), seg=seg, pre={})
