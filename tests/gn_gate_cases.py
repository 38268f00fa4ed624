"""Crafted inputs for the correspondence gates of the Gauss-Newton tracker (Core/Cuda/reduce.cu:292-353 search(), :812-895 RGBResidual, :547-626
RGBReduction), each built to sit ON one decision: the rounded projection, the 0.10 m gate, the sin 20 degrees gate, the NaN tests, the border /
window / gradient / depth tests of the photometric term, the weight's epsilon.  Plain numpy: nothing here imports the product or the oracle, so a
case is the same input for every implementation held to it (tests/test_gn_gates_host.py, tests/test_gpu_gn_gates.py).

An ICP case is ONE candidate pixel: a current vertex / normal, a model vertex / normal at the pixel the vertex projects to, the decision it expects
(1 inlier or 0) and its PREMISES -- the facts, evaluated here in float32 operation by operation (eval_icp), that make the case bite ("fl(d.d) ==
dist2Max").  tests/test_gn_gates_host.py asserts every premise; a case that stops sitting on its boundary then fails loudly instead of passing
emptily.  dist2Max / sine2Min are computed here from their definition (max{y : sqrtf(y) <= T}, min{y : sqrtf(y) >= S}) with numpy's correctly
rounded float32 sqrt, never read from the product.

`undefined`: the float32 projection of a FINITE vertex is NaN or infinite.  The reference converts it with __float2int_rn; every CPU build of that
text converts with a cast, which the language leaves undefined there.  Such cases are detected here, kept out of every comparison and listed by
name (UNDEFINED_NAMES).  A NaN vertex is not among them: whatever pixel it is given, its distance to the model is NaN and it is rejected.
"""
from collections import namedtuple

import numpy as np

F = np.float32
NAN = F(np.nan)
DIST = F(0.10)
ANGLE = F(np.sin(np.float32(20.0 * 3.14159254 / 180.0)))   # the tests' usual thresholds (tests/test_gpu_kernels.py::test_icp_step)
FX = FY = F(20.0)


def up(v, n=1):
    v = F(v)
    for _ in range(n):
        v = np.nextafter(v, F(np.inf))
    return v


def down(v, n=1):
    v = F(v)
    for _ in range(n):
        v = np.nextafter(v, F(-np.inf))
    return v


def dist2_max(T):
    """max{y : sqrtf(y) <= T}"""
    T = F(T)
    y = F(T * T)
    while np.sqrt(y) > T:
        y = down(y)
    while np.sqrt(up(y)) <= T:
        y = up(y)
    return y


def sine2_min(S):
    """min{y : sqrtf(y) >= S}"""
    S = F(S)
    y = F(S * S)
    while np.sqrt(y) < S:
        y = up(y)
    while y > 0 and np.sqrt(down(y)) >= S:
        y = down(y)
    return y


D2MAX = dist2_max(DIST)
S2MIN = sine2_min(ANGLE)

# ------------------------------------------------------------------------------------------------------------------------------------------
# float32 arithmetic of search(), one rounding per operation, in the reference's order (m33_mul: (R0 x + R1 y) + R2 z)
# ------------------------------------------------------------------------------------------------------------------------------------------
Pose = namedtuple("Pose", "name Rcurr tcurr Rpi tprev")


def _rot_xyz(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


IDENT = Pose("I", np.eye(3, dtype=F), np.zeros(3, F), np.eye(3, dtype=F), np.zeros(3, F))
# Rcurr, tcurr of test_icp_step; the previous pose keeps the identity rotation and gets a translation
MOVED = Pose("P", _rot_xyz(0.004, -0.003, 0.002).astype(F), np.array([0.003, -0.002, 0.001], F), np.eye(3, dtype=F),
             np.array([0.01, -0.02, 0.005], F))


def mul33(R, v):
    R = np.asarray(R, F).reshape(9)
    x, y, z = F(v[0]), F(v[1]), F(v[2])
    with np.errstate(all="ignore"):
        return np.array([F(F(F(R[0] * x) + F(R[1] * y)) + F(R[2] * z)), F(F(F(R[3] * x) + F(R[4] * y)) + F(R[5] * z)),
                         F(F(F(R[6] * x) + F(R[7] * y)) + F(R[8] * z))], F)


def dot3(a, b):
    with np.errstate(all="ignore"):
        return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def cross3(a, b):
    with np.errstate(all="ignore"):
        return np.array([F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])), F(F(a[0] * b[1]) - F(a[1] * b[0]))], F)


def to_global(pose, v):
    with np.errstate(all="ignore"):
        return (mul33(pose.Rcurr, v) + pose.tcurr).astype(F)


def project(pose, v, cx, cy):
    """(projection x, projection y before rounding, vcurr_cp.z, vcurr_g), all float32"""
    with np.errstate(all="ignore"):
        g = to_global(pose, v)
        cp = mul33(pose.Rpi, (g - pose.tprev).astype(F))
        px = F(F(F(cp[0] * FX) / cp[2]) + F(cx))
        py = F(F(F(cp[1] * FY) / cp[2]) + F(cy))
    return px, py, cp[2], g


def rn(v):
    """__float2int_rn on a finite float32: round half to even"""
    return int(np.rint(np.float64(v)))


# ------------------------------------------------------------------------------------------------------------------------------------------
# (A) ICP: one candidate pixel per case
# ------------------------------------------------------------------------------------------------------------------------------------------
IcpCase = namedtuple("IcpCase", "name pose expect undefined premise vcurr ncurr target vprev nprev")
UP_N = np.array([0, 0, -1], F)


def eval_icp(c, W, H, cx, cy):
    """what search() computes for the case's pixel, in float32: dict(px, py, z, ux, uy, inside, dist2, sine2)"""
    px, py, z, g = project(c.pose, c.vcurr, cx, cy)
    out = dict(px=px, py=py, z=z, ux=None, uy=None, inside=False, dist2=None, sine2=None)
    if np.isfinite(px) and np.isfinite(py):
        out["ux"], out["uy"] = rn(px), rn(py)
        out["inside"] = 0 <= out["ux"] < W and 0 <= out["uy"] < H
    if c.vprev is not None:
        with np.errstate(all="ignore"):
            dv = (np.asarray(c.vprev, F) - g).astype(F)
            out["dist2"] = dot3(dv, dv)
            cr = cross3(mul33(c.pose.Rcurr, c.ncurr), np.asarray(c.nprev, F))
            out["sine2"] = dot3(cr, cr)
    return out


class Geometry:
    """frame size, principal point (integer) and the model pixels already taken"""

    def __init__(self, W, H):
        self.W, self.H, self.cx, self.cy = W, H, W // 2, H // 2
        self.used = {(0, 0)}              # (0, 0): where a NaN projection lands under the reference's conversion -- kept for the NaN-vertex case
        self._k = 0

    def K(self):
        return float(FX), float(FY), float(self.cx), float(self.cy)

    def take(self, tx=None, ty=None):
        """an unused model pixel with the given column and / or row, away from the image border unless a coordinate is given there"""
        W, H = self.W, self.H
        for _ in range(W * H):
            self._k += 1
            x = tx if tx is not None else 3 + (self._k * 7) % (W - 6)
            y = ty if ty is not None else 3 + (self._k * 5 + self._k // (W - 6)) % (H - 6)
            if (x, y) not in self.used:
                self.used.add((x, y))
                return x, y
        raise AssertionError("no free model pixel")


def _vertex_to(G, tx, ty, z):
    """a vertex at depth z whose projection under the identity pose lies within 1e-3 px of the centre of pixel (tx, ty)"""
    return np.array([F((tx - G.cx) * float(z) / float(FX)), F((ty - G.cy) * float(z) / float(FY)), F(z)], F)


def _search_offset(g, axis, target, side_axis):
    """model vertex p with fl(|p - g|^2) == target, the offset along `axis` (about +sqrt(target)); a second small component along side_axis
    (multiples of 2^-20 up to 2e-3) is added only where no single-axis offset squares to the target.  g: vcurr_g (float32).
    Returns (p, components used).  fl(|dv|^2) = fl(fl(a a) + fl(b b)) whatever the axes: the third product is 0 and adding 0 is exact."""
    root = F(np.sqrt(np.float64(target)))
    base = F(g[axis] + root)
    cand_a = [base]
    for k in range(1, 48):
        cand_a += [up(base, k), down(base, k)]
    steps = (F(g[side_axis]) + np.arange(0, 2048, dtype=np.float64) * 2.0 ** -20).astype(F)
    for two in (False, True):
        for pa in cand_a:
            da = F(pa - g[axis])
            db = (steps - F(g[side_axis])).astype(F) if two else np.zeros(1, F)
            d2 = (F(da * da) + db * db).astype(F)
            hit = np.nonzero(d2 == target)[0]
            if len(hit):
                p = np.array(g, F)
                p[axis] = pa
                if two:
                    p[side_axis] = steps[hit[0]]
                dv = (p - g).astype(F)
                assert dot3(dv, dv) == target
                return p, (2 if two and db[hit[0]] != 0 else 1)
    raise AssertionError("no offset found")


def _dist_cases(G, pose, tag):
    out = []
    for axis, an in ((0, "x"), (1, "y"), (2, "z")):
        for which, target, expect in (("at", D2MAX, 1), ("above", up(D2MAX), 0), ("below", down(D2MAX), 1)):
            if pose is IDENT:
                # the current vertex sits where the subtraction is exact: component 0 on the principal column / row, 2^-6 in depth (its sum with
                # 0.1 stays inside [2^-4, 2^-3), where both are multiples of 2^-27)
                if axis == 0:
                    tx, ty = G.take(tx=G.cx)
                    v = _vertex_to(G, tx, ty, 1.0); v[0] = F(0)
                elif axis == 1:
                    tx, ty = G.take(ty=G.cy)
                    v = _vertex_to(G, tx, ty, 1.0); v[1] = F(0)
                else:
                    tx, ty = G.take()
                    v = _vertex_to(G, tx, ty, 2.0 ** -6)
            else:
                if axis != 0:
                    continue              # (the moved pose repeats the trio once: the offset search already spans two components)
                tx, ty = G.take()
                v = _vertex_to(G, tx, ty, 1.0)
                px, py, _, _ = project(pose, v, G.cx, G.cy)
                G.used.discard((tx, ty))
                tx, ty = rn(px), rn(py)
                assert (tx, ty) not in G.used
                G.used.add((tx, ty))
            g = to_global(pose, v)
            p, ncomp = _search_offset(g, axis, target, (axis + 1) % 3)
            c = IcpCase(f"dist_{an}_{which}{tag}", pose, expect, False, [], v, UP_N, (tx, ty), p, mul33(pose.Rcurr, UP_N))
            e = eval_icp(c, G.W, G.H, G.cx, G.cy)
            c.premise.append((f"fl(|vprev - vcurr_g|^2) == {'dist2Max' if which == 'at' else which + ' dist2Max by one ulp'}", e["dist2"] == target))
            c.premise.append(("sqrtf of it is %s the threshold" % ("above" if which == "above" else "not above"),
                              bool(np.sqrt(e["dist2"]) > DIST) == (which == "above")))
            c.premise.append(("projects into its model pixel", e["inside"] and (e["ux"], e["uy"]) == (tx, ty)))
            c.premise.append(("normals parallel", e["sine2"] == 0))
            if which == "at" and pose is IDENT:
                c.premise.append(("a single-axis offset of 0.1f squares to dist2Max", ncomp == 1 and F(p[axis] - g[axis]) == DIST))
            out.append(c)
    return out


def _angle_pair(target):
    """(a, b) with fl(fl(b b) + fl(a a)) == target: a a few ulps below sqrt(target), b a multiple of 2^-18"""
    root = F(np.sqrt(np.float64(target)))
    for ka in range(0, 64):
        a = down(root, ka)
        for kb in range(0, 4096):
            b = F(kb * 2.0 ** -18)
            if F(F(b * b) + F(a * a)) == target:
                return a, b
    raise AssertionError("no normal pair found")


def _angle_cases(G):
    out = []
    for which, target, expect in (("at", S2MIN, 0), ("below", down(S2MIN), 1), ("parallel", F(0), 1)):
        tx, ty = G.take()
        v = _vertex_to(G, tx, ty, 1.0)
        a, b = (F(0), F(0)) if which == "parallel" else _angle_pair(target)
        c = IcpCase(f"angle_{which}", IDENT, expect, False, [], v, UP_N, (tx, ty), v.copy(), np.array([a, b, -1], F))
        e = eval_icp(c, G.W, G.H, G.cx, G.cy)
        c.premise.append((f"sine^2 == {'sine2Min' if which == 'at' else 'the float below sine2Min' if which == 'below' else '0'}", e["sine2"] == target))
        if which != "parallel":
            c.premise.append(("sqrtf of it is %s the threshold" % ("not below" if which == "at" else "below"), bool(np.sqrt(e["sine2"]) < ANGLE) == (which == "below")))
        c.premise.append(("distance 0, projects into its model pixel", e["dist2"] == 0 and (e["ux"], e["uy"]) == (tx, ty)))
        out.append(c)
    return out


def _proj_vertex(G, px, py):
    """a vertex at depth 20 (= fx = fy: x fx / z == x exactly) whose projection is exactly (px, py) for half-integer px, py"""
    return np.array([F(px - G.cx), F(py - G.cy), F(20.0)], F)


def _proj_cases(G):
    out = []
    W, H = G.W, G.H

    def add(name, v, lands, extra, trap=None):
        # trap: a projection that rounds out of the image has no model pixel; where the pixel index it WOULD address (uy W + ux) lies inside the map,
        # that pixel holds a matching model vertex, so that a bounds test one off (ux >= W read as ux > W, ux < 0 dropped) finds an inlier there
        for pxl in (lands, trap):
            if pxl is not None:
                assert pxl not in G.used, (name, pxl)
                G.used.add(pxl)
        at = lands if lands is not None else trap
        c = IcpCase(name, IDENT, 1 if lands is not None else 0, False, [], v, UP_N, at, v.copy() if at is not None else None, UP_N)
        e = eval_icp(c, W, H, G.cx, G.cy)
        c.premise.extend(extra(e))
        if lands is not None:
            c.premise.append(("rounds into the model pixel", e["inside"] and (e["ux"], e["uy"]) == lands))
        else:
            c.premise.append(("rounds out of the image", e["ux"] is not None and not e["inside"]))
            if trap is not None:
                c.premise.append(("the index it would address is the trap pixel's", e["uy"] * W + e["ux"] == trap[1] * W + trap[0]))
        out.append(c)

    for axis, an, size in ((0, "x", W), (1, "y", H)):
        def P(t, free):
            return (t, free) if axis == 0 else (free, t)

        def V(t, free):
            return _proj_vertex(G, *P(t, free + 0.0))

        tie = lambda t: (lambda e: [(f"projection is exactly {t}", float(e["px" if axis == 0 else "py"]) == t)])
        free = [3 + 2 * axis, 5 + 2 * axis, 7 + 2 * axis, 9 + 2 * axis, 11 + 2 * axis, 13 + 2 * axis, 15 + 2 * axis]
        add(f"tie_{an}_even", V(2.5, free[0]), P(2, free[0]), tie(2.5))
        add(f"tie_{an}_odd", V(3.5, free[1]), P(4, free[1]), tie(3.5))
        add(f"edge_{an}_minus_half", V(-0.5, free[2]), P(0, free[2]), tie(-0.5))
        add(f"edge_{an}_size_minus_1p5", V(size - 1.5, free[3]), P(size - 2, free[3]), tie(size - 1.5))
        add(f"edge_{an}_size_minus_half", V(size - 0.5, free[4]), None, tie(size - 0.5), trap=(0, free[4] + 1) if axis == 0 else None)
        v = V(-0.5, free[5])
        v[axis] = down(v[axis])
        add(f"edge_{an}_below_minus_half", v, None,
            lambda e: [("projection is just below -0.5", -0.5 - 1e-4 < float(e["px" if axis == 0 else "py"]) < -0.5)],
            trap=(W - 1, free[5] - 1) if axis == 0 else None)
    # the depth test: vcurr_cp.z negative (its projection is the mirror image's: inside), tiny positive, zero
    tx, ty = G.take()
    v = _vertex_to(G, tx, ty, 1.0)
    vneg = np.array([-v[0], -v[1], F(-1.0)], F)
    cneg = IcpCase("z_negative", IDENT, 0, False, [], vneg, UP_N, (tx, ty), vneg.copy(), UP_N)
    e = eval_icp(cneg, W, H, G.cx, G.cy)
    cneg.premise.extend([("projects into its model pixel, distance 0, normals parallel", (e["ux"], e["uy"]) == (tx, ty) and e["dist2"] == 0 and e["sine2"] == 0),
                         ("vcurr_cp.z < 0", e["z"] < 0)])
    out.append(cneg)
    tx, ty = G.take(tx=G.cx, ty=G.cy) if (G.cx, G.cy) not in G.used else (None, None)
    assert tx is not None
    vt = np.array([0, 0, 1e-30], F)
    ct = IcpCase("z_tiny_positive", IDENT, 1, False, [], vt, UP_N, (tx, ty), vt.copy(), UP_N)
    e = eval_icp(ct, W, H, G.cx, G.cy)
    ct.premise.append(("0 / 1e-30 projects onto the principal point", (e["ux"], e["uy"]) == (G.cx, G.cy) and 0 < float(e["z"]) < 1e-29))
    out.append(ct)
    for name, v in (("z_negative_zero", np.array([0.25, 0.25, -0.0], F)), ("z_zero_on_axis", np.array([0, 0, 0], F)),
                    ("z_denormal_overflow", np.array([0.25, 0.25, 1e-45], F))):
        c = IcpCase(name, IDENT, 0, True, [], v, UP_N, (0, 0), v.copy(), UP_N)
        e = eval_icp(c, W, H, G.cx, G.cy)
        c.premise.append(("the float32 projection is not finite", not (np.isfinite(e["px"]) and np.isfinite(e["py"]))))
        out.append(c)
    return out


def _nan_cases(G):
    out = []
    for name, who, comp, expect in (("nan_ncurr_x", "ncurr", 0, 0), ("nan_ncurr_y_only", "ncurr", 1, 0), ("nan_nprev_x", "nprev", 0, 0),
                                    ("nan_nprev_y_only", "nprev", 1, 0), ("nan_vprev", "vprev", None, 0), ("nan_vcurr", "vcurr", None, 0)):
        tx, ty = (0, 0) if who == "vcurr" else G.take()
        v = _vertex_to(G, tx, ty, 1.0)
        d = dict(vcurr=v.copy(), ncurr=UP_N.copy(), vprev=v.copy(), nprev=UP_N.copy())
        if comp is None:
            d[who][:] = NAN
            if who == "vcurr":
                d["vprev"] = np.array([0, 0, 1], F)
        else:
            d[who][comp] = NAN
        c = IcpCase(name, IDENT, expect, False, [], d["vcurr"], d["ncurr"], (tx, ty), d["vprev"], d["nprev"])
        e = eval_icp(c, G.W, G.H, G.cx, G.cy)
        if who == "vcurr":
            c.premise.append(("the distance is NaN whatever pixel the vertex is given", np.isnan(e["dist2"])))
        else:
            c.premise.append(("projects into its model pixel", (e["ux"], e["uy"]) == (tx, ty)))
            # (only x is tested by the reference: a NaN in y alone reaches the sums through sine^2 = NaN, which fails `sine < angleThres`)
            c.premise.append(("the gate that rejects it", {"ncurr": np.isnan(e["sine2"]), "nprev": np.isnan(e["sine2"]), "vprev": np.isnan(e["dist2"])}[who]))
        out.append(c)
    return out


def _pose_tie_case(G):
    """a tie at k + 0.5 along x after the moved pose's transform: the vertex's x is searched ulp by ulp until the float32 projection is exact"""
    for _ in range(16):
        tx, ty = G.take()
        tx -= tx % 2                                         # even k: the tie must go DOWN to k
        v = _vertex_to(G, tx, ty, 1.0)
        for _ in range(4):                                   # onto the tie to within a few ulps, then ulp by ulp
            px, _, _, _ = project(MOVED, v, G.cx, G.cy)
            v[0] = F(v[0] + F((tx + 0.5 - float(px)) / float(FX)))
        cand = v.copy()
        for k, step in ((k, s) for k in range(1 << 12) for s in (up, down)):
            cand[0] = step(v[0], k)
            px, py, _, _ = project(MOVED, cand, G.cx, G.cy)
            if float(px) == tx + 0.5:
                break
        else:
            continue
        lands = (tx, rn(py))
        if lands in G.used:
            continue
        G.used.add(lands)
        c = IcpCase("tie_x_even_P", MOVED, 1, False, [], cand.copy(), UP_N, lands, to_global(MOVED, cand), mul33(MOVED.Rcurr, UP_N))
        e = eval_icp(c, G.W, G.H, G.cx, G.cy)
        c.premise.extend([(f"projection is exactly {tx + 0.5} after the transform", float(e["px"]) == tx + 0.5),
                          ("rounds down into the model pixel", (e["ux"], e["uy"]) == lands), ("distance 0", e["dist2"] == 0),
                          ("normals parallel", e["sine2"] == 0)])
        return c
    raise AssertionError("no tie found")


def icp_cases(W=32, H=24):
    """(geometry, cases) for a W x H frame; every case owns a model pixel"""
    G = Geometry(W, H)
    cases = _proj_cases(G) + _dist_cases(G, IDENT, "") + _angle_cases(G) + _nan_cases(G) + _dist_cases(G, MOVED, "_P") + [_pose_tie_case(G)]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:      # the only exclusion: detected, not declared
        px, py, _, _ = project(c.pose, c.vcurr, G.cx, G.cy)
        assert c.undefined == (bool(np.isfinite(c.vcurr).all()) and not (np.isfinite(px) and np.isfinite(py))), c.name
    return G, cases


UNDEFINED_NAMES = ["z_negative_zero", "z_zero_on_axis", "z_denormal_overflow"]


def icp_frame(G, cases, cur_index=None):
    """vertex / normal maps of the frame and of the model, NaN except where the cases live.  cur_index[k]: pixel index of case k's current vertex
    (default: its own model pixel).  All cases must share one pose."""
    W, H = G.W, G.H
    P = W * H
    vc, nc, vp, npv = (np.full((3, P), np.nan, F) for _ in range(4))
    assert len({c.pose.name for c in cases}) <= 1
    for k, c in enumerate(cases):
        i = int(cur_index[k]) if cur_index is not None else (c.target[1] * W + c.target[0]) if c.target is not None else W + 1
        assert np.isnan(nc[0, i]) and np.isnan(nc[1, i]) and np.isnan(vc[2, i]), "two cases on one pixel"
        vc[:, i] = c.vcurr
        nc[:, i] = c.ncurr
        if c.vprev is not None:
            j = c.target[1] * W + c.target[0]
            vp[:, j] = c.vprev
            npv[:, j] = c.nprev
    return [a.reshape(3, H, W) for a in (vc, nc, vp, npv)]


def spread(n, P):
    """n distinct pixel indices over the whole range [0, P), first and last pixel included"""
    idx = np.unique(np.round(np.linspace(0, P - 1, n)).astype(np.int64))
    assert len(idx) == n
    return idx


def own_pixels(G, cases):
    """for each case the pixel whose ray its current vertex lies on (to within the half pixel of a tie; clamped into the image; a vertex without a
    finite projection gets a free pixel): where a frame's vertex map -- a back-projection of its depth image -- would hold it"""
    taken, out = set(), []
    for c in cases:
        px, py, _, _ = project(IDENT, c.vcurr, G.cx, G.cy)
        i = (min(max(rn(py), 0), G.H - 1) * G.W + min(max(rn(px), 0), G.W - 1)) if np.isfinite(px) and np.isfinite(py) else G.W + 1
        while i in taken:
            i += 1
        taken.add(i)
        out.append(i)
    return np.array(out, np.int64)


def minefields(W, H, pins=(), on_ray=False):
    """[(name, pose, cases, frame maps, current indices, expected count)]: the accepted and the rejected cases of each pose in one frame each.
    The current vertices lie evenly over the whole index range, first and last pixel included; pins: pixel indices that must carry a case (the
    caller knows which slots and workgroups of its launch form they are).  on_ray: every current vertex at the pixel whose ray it lies on instead
    (own_pixels) -- the batched pixel pass's slab culling is stated for vertex maps that are back-projections."""
    G, cases = icp_cases(W, H)
    out = []
    for pose in (IDENT, MOVED):
        for expect in (1, 0):
            sel = [c for c in cases if c.pose is pose and c.expect == expect and not c.undefined]
            idx = own_pixels(G, sel) if on_ray else spread(len(sel), W * H)
            free = [k for k in range(1, len(idx) - 1)]
            for pin in (() if on_ray else pins):
                if len(idx) >= 3 and int(pin) not in idx and free:
                    idx[free.pop(len(free) // 2)] = int(pin)
            assert len(set(idx.tolist())) == len(idx)
            out.append((f"{'accept' if expect else 'reject'}_{pose.name}", pose, sel, icp_frame(G, sel, idx), idx, len(sel) if expect else 0))
    return G, out


def normals_rect(npv):
    """{x0, y0, x1, y1} of the model pixels that hold a normal (what the batched model pyramid leaves in TrackModelDev::rect)"""
    ys, xs = np.nonzero(~np.isnan(npv[0]))
    return np.array([xs.min(), ys.min(), xs.max(), ys.max()], np.int32)


def pack_system(A, b, res):
    """the oracle's (A, b, {sum r^2, inliers}) in the device's order: 27 upper-triangle products, sum r^2, inliers"""
    out = []
    for i in range(6):
        for j in range(i, 7):
            out.append(b[i] if j == 6 else A[i, j])
    return np.array(out + [res[0], res[1]], np.float64)


# ------------------------------------------------------------------------------------------------------------------------------------------
# (B) photometric residual: frames built directly
# ------------------------------------------------------------------------------------------------------------------------------------------
RgbCase = namedtuple("RgbCase", "name expect px minScale dIdx dIdy lastDepth nextDepth lastImage nextImage kt krk premise")
DELTA = F(0.07)


def _rgb_blank(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return dict(minScale=F(100.0), dIdx=np.full((H, W), 30, np.int16), dIdy=np.full((H, W), 40, np.int16), lastDepth=np.ones((H, W), F),
                nextDepth=np.full((H, W), np.nan, F), lastImage=(1 + (xx * 7 + yy * 13) % 199).astype(np.uint8), nextImage=np.full((H, W), 200, np.uint8),
                kt=np.zeros(3, F), krk=np.eye(3, dtype=F))


def rgb_cases(W=32, H=24):
    """One candidate pixel per case (the next depth is NaN everywhere else).  expect: (valid, u0, v0) or (0, None, None)."""
    out = []

    def add(name, x, y, expect, edit=None, premise=None, d1=1.0):
        f = _rgb_blank(W, H)
        f["nextDepth"][y, x] = F(d1)
        if edit:
            edit(f)
        u0, v0 = expect[1:] if expect[0] else (None, None)
        out.append(RgbCase(name, (int(expect[0]), u0, v0), (x, y), f["minScale"], f["dIdx"], f["dIdy"], f["lastDepth"], f["nextDepth"], f["lastImage"],
                           f["nextImage"], f["kt"], f["krk"], list(premise(f) if premise else [])))

    X, Y = 10, 10
    add("valid_plain", X, Y, (1, X, Y))
    # border: x < W - 5 and y < H - 1
    add("border_x_last_inside", W - 6, Y, (1, W - 6, Y))
    add("border_x_first_outside", W - 5, Y, (0,))
    add("border_y_last_inside", X, H - 2, (1, X, H - 2))
    add("border_y_first_outside", X, H - 1, (0,))
    # 4 x 4 window [x - 2, x + 1] x [y - 2, y + 1] of the next image: a zero texel at a corner kills, one just outside does not
    def zero(px, py):
        return lambda f: f["nextImage"].__setitem__((py, px), 0)
    for n, (dx, dy) in (("tl", (-2, -2)), ("tr", (1, -2)), ("bl", (-2, 1)), ("br", (1, 1))):
        add(f"window_corner_{n}", X, Y, (0,), zero(X + dx, Y + dy))
    for n, (dx, dy) in (("left", (-3, 0)), ("right", (2, 0)), ("top", (0, -3)), ("bottom", (0, 2))):
        add(f"window_outside_{n}", X, Y, (1, X, Y), zero(X + dx, Y + dy))
    # clamped windows: at x = 1 the window is columns 0..2, at x = 0 columns 0..1 (and the same for rows)
    add("window_clamped_x1_col0", 1, Y, (0,), zero(0, Y))
    add("window_clamped_x1_col2", 1, Y, (0,), zero(2, Y))
    add("window_clamped_x1_col3", 1, Y, (1, 1, Y), zero(3, Y))
    add("window_clamped_x0_col1", 0, Y, (0,), zero(1, Y))
    add("window_clamped_x0_col2", 0, Y, (1, 0, Y), zero(2, Y))
    add("window_clamped_y1_row0", X, 1, (0,), zero(X, 0))
    add("window_clamped_y1_row2", X, 1, (0,), zero(X, 2))
    add("window_clamped_y1_row3", X, 1, (1, X, 1), zero(X, 3))
    add("window_clamped_y0_row1", X, 0, (0,), zero(X, 1))
    add("window_clamped_y0_row2", X, 0, (1, X, 0), zero(X, 2))
    # gradient: (float)(valx^2 + valy^2) >= minScale
    def grad(gx, gy, ms):
        def edit(f):
            f["dIdx"][Y, X], f["dIdy"][Y, X], f["minScale"] = gx, gy, F(ms)
        return edit
    add("gradient_at", X, Y, (1, X, Y), grad(3, 4, 25.0))
    add("gradient_threshold_above", X, Y, (0,), grad(3, 4, up(25.0)))
    add("gradient_threshold_below", X, Y, (1, X, Y), grad(3, 4, down(25.0)))
    add("gradient_negative", X, Y, (1, X, Y), grad(-3, 4, 25.0))
    big = 4097 * 4097 + 2 * 2                           # 16 785 413: odd and above 2^24, half way between two floats -- the int -> float conversion rounds to even
    add("gradient_big_at", X, Y, (1, X, Y), grad(4097, 2, F(big)), lambda f: [("the squared sum is above 2^24 and no float", big > 2 ** 24 and float(F(big)) != big)])
    add("gradient_big_above", X, Y, (0,), grad(4097, 2, up(F(big))))
    add("d1_nan", X, Y, (0,), lambda f: f["nextDepth"].__setitem__((Y, X), np.nan))
    # u0 / v0 ties through kt = (k + 0.5) d1
    def kt(ax, v):
        return lambda f: f["kt"].__setitem__(ax, F(v))
    add("u0_tie_even", 10, Y, (1, 10, Y), kt(0, 0.5))
    add("u0_tie_odd", 11, Y, (1, 12, Y), kt(0, 0.5))
    add("u0_minus_half", 0, Y, (1, 0, Y), kt(0, -0.5))
    add("u0_size_minus_half", W - 6, Y, (0,), kt(0, 5.5))
    add("u0_size_minus_1p5", W - 6, Y, (1, W - 2, Y), kt(0, 4.5))
    add("v0_tie_even", X, 10, (1, X, 10), kt(1, 0.5))
    add("v0_tie_odd", X, 11, (1, X, 12), kt(1, 0.5))
    add("v0_minus_half", X, 0, (1, X, 0), kt(1, -0.5))
    add("v0_size_minus_half", X, H - 2, (0,), kt(1, 1.5))
    add("v0_size_minus_1p5", X, H - 3, (1, X, H - 2), kt(1, 1.5))
    # d0 > 0 (d1 = 0.05: |td1 - d0| <= 0.07 holds for every d0 in [0, 0.05], so only the sign test decides)
    def d0(v):
        return lambda f: f["lastDepth"].__setitem__((Y, X), v)
    add("d0_zero", X, Y, (0,), d0(F(0)), d1=0.05)
    add("d0_negative_zero", X, Y, (0,), d0(F(-0.0)), d1=0.05)
    add("d0_nan", X, Y, (0,), d0(NAN), d1=0.05)
    add("d0_smallest_denormal", X, Y, (1, X, Y), d0(F(1e-45)), lambda f: [("d0 is the smallest denormal", f["lastDepth"][Y, X] == np.nextafter(F(0), F(1)))], d1=0.05)
    add("last_image_zero", X, Y, (0,), lambda f: f["lastImage"].__setitem__((Y, X), 0))
    # |td1 - d0| <= 0.07f: with d1 = 2^-7 the sum 2^-7 + 0.07f is exact, and so are its neighbours' differences
    lo, hi = F(2.0 ** -7), F(F(2.0 ** -7) + DELTA)
    exact = lambda a, b, want: (lambda f: [("|td1 - d0| is " + want, {"0.07f": F(abs(F(a - b))) == DELTA, "above": F(abs(F(a - b))) == up(DELTA),
                                                                       "below": F(abs(F(a - b))) == down(DELTA)}[want.split()[0]]),
                                           ("the sum is exact", np.float64(lo) + np.float64(DELTA) == np.float64(hi))])
    add("depth_delta_at_far", X, Y, (1, X, Y), d0(hi), exact(lo, hi, "0.07f"), d1=lo)
    add("depth_delta_above_far", X, Y, (0,), d0(up(hi)), exact(lo, up(hi), "above by one ulp"), d1=lo)
    add("depth_delta_below_far", X, Y, (1, X, Y), d0(down(hi)), exact(lo, down(hi), "below by one ulp"), d1=lo)
    add("depth_delta_at_near", X, Y, (1, X, Y), d0(lo), exact(hi, lo, "0.07f"), d1=hi)
    add("depth_delta_above_near", X, Y, (0,), d0(lo), exact(up(hi), lo, "above by one ulp"), d1=up(hi))
    add("depth_delta_below_near", X, Y, (1, X, Y), d0(lo), exact(down(hi), lo, "below by one ulp"), d1=down(hi))
    # the largest |diff| a valid correspondence can carry: both images must be non-zero at their pixels, so 255 - 1 and 1 - 255
    def img(nv, lv):
        def edit(f):
            f["nextImage"][Y, X], f["lastImage"][Y, X] = nv, lv
        return edit
    add("diff_plus_254", X, Y, (1, X, Y), img(255, 1))
    add("diff_minus_254", X, Y, (1, X, Y), img(1, 255))
    assert len({c.name for c in out}) == len(out)
    return out


def rgb_gate_numpy(img, dIdx, dIdy, minScale):
    """the three pose-independent tests of RGBResidual::getProducts (reduce.cu:823-851) as a gate image: x < W - 5 and y < H - 1, no zero texel in
    rows [y - 2, y + 1] x columns [x - 2, x + 1] clipped to the image, (float)(dIdx^2 + dIdy^2) >= minScale"""
    H, W = img.shape
    zero = np.zeros((H + 4, W + 4), bool)                 # padded by 2: texels outside the image are no texels
    zero[2:H + 2, 2:W + 2] = img == 0
    hit = np.zeros((H, W), bool)
    for dy in (-2, -1, 0, 1):
        for dx in (-2, -1, 0, 1):
            hit |= zero[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
    m2 = (dIdx.astype(np.int32) ** 2 + dIdy.astype(np.int32) ** 2).astype(F)
    g = ~hit & (m2 >= F(minScale))
    g[H - 1:, :] = False
    g[:, W - 5:] = False
    return g.astype(np.uint8)


def texture(W, H, seed):
    """a grey image for the gate kernels: smooth enough that many pixels share a gradient magnitude, with zero texels (singles, the image corners, a
    block) whose 4 x 4 neighbourhoods cross every tile edge of a 32-pixel tiling"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = (100 + 60 * np.sin(xx / 5.0) * np.cos(yy / 7.0) + rng.integers(0, 3, (H, W))).astype(np.uint8)
    for _ in range(max(6, W * H // 400)):
        img[rng.integers(0, H), rng.integers(0, W)] = 0
    for x in range(29, W, 32):
        for y in range(30, H, 32):
            img[y, x] = 0
            img[min(y + 3, H - 1), min(x + 4, W - 1)] = 0
    img[0, 0] = img[H - 1, W - 1] = img[0, W - 1] = img[H - 1, 0] = 0
    return img


def rgb_field(W, H):
    """All (B) cases with krk = I, kt = 0 whose pixel is not tied to the image border, each at a place of its own in one W x H frame (placed over the
    whole index range), plus the four border cases at the frame's own border.  Returns (frame dict, [(name, (x, y), expect)])."""
    small = [c for c in rgb_cases(32, 24) if not c.kt.any() and c.px == (10, 10)]
    f = _rgb_blank(W, H)
    f["minScale"] = F(25.0)
    f["dIdx"][:], f["dIdy"][:] = 3, 4                    # every pixel AT the gradient threshold
    placed = []
    cols, rows = (W - 16) // 8, (H - 8) // 8
    slots = [(6 + 8 * i, 4 + 8 * j) for j in range(rows) for i in range(cols)]
    pick = spread(len(small), len(slots))
    for c, s in zip(small, pick):
        x, y = slots[s]
        for key in ("dIdx", "dIdy", "lastDepth", "nextDepth", "lastImage", "nextImage"):
            src = getattr(c, key)
            f[key][y - 3:y + 4, x - 3:x + 4] = src[7:14, 7:14]
        ms = float(c.minScale)
        gx, gy = int(c.dIdx[10, 10]), int(c.dIdy[10, 10])
        if ms != 100.0:        # a gradient case: the frame has ONE minScale (25), so the case keeps its side of it
            valid = float(F(gx * gx + gy * gy)) >= ms
            f["dIdx"][y, x], f["dIdy"][y, x] = (3, 4) if valid else (3, 3)
        else:
            f["dIdx"][y, x], f["dIdy"][y, x] = 3, 4
        placed.append((c.name, (x, y), c.expect[0]))
    for name, (x, y), e in (("border_x_last_inside", (W - 6, 3), 1), ("border_x_first_outside", (W - 5, 5), 0), ("border_y_last_inside", (3, H - 2), 1),
                            ("border_y_first_outside", (5, H - 1), 0), ("first_pixel", (0, 0), 1), ("last_inside_pixel", (W - 6, H - 2), 1)):
        f["nextDepth"][y, x] = 1.0
        placed.append((name, (x, y), e))
    return f, placed


# ------------------------------------------------------------------------------------------------------------------------------------------
# (C) the photometric weight: w = sigma + |diff|; w > 1.1920929e-07f ? 1 / w : 1; sigma == -1: w = 1 (reduce.cu:566-571)
# ------------------------------------------------------------------------------------------------------------------------------------------
EPS = F(1.1920929e-07)
SIGMAS = [("zero", F(0)), ("epsilon", EPS), ("above_epsilon", up(EPS)), ("minus_one", F(-1))]   # w = 1, 1 (not greater), ~8.4e6, 1


def weight_case(W=32, H=24):
    """a single correspondence with diff == 0, so that w is a function of sigma alone"""
    c = [c for c in rgb_cases(W, H) if c.name == "valid_plain"][0]
    x, y = c.px
    c.nextImage[y, x] = c.lastImage[y, x]
    return c


def row_minus_one_trap(G, c, maps):
    """For a case whose projection rounds to row -1 inside the columns: the pixel index uy W + ux is negative, so a dropped `uy < 0` would read W - ux
    floats IN FRONT of each plane of the model maps.  Returns (pad_v, pad_n, maps): W floats to place in front of the model's vertex / normal map
    and maps whose last row holds the rest, such that exactly that read finds the case's own vertex and normal -- an inlier only for code that
    addresses row -1.  (In front of plane 0 lies the pad; in front of planes 1 and 2 lie the last rows of planes 0 and 1.)"""
    W, H = G.W, G.H
    e = eval_icp(c, W, H, G.cx, G.cy)
    assert e["uy"] == -1 and 0 <= e["ux"] < W and c.expect == 0
    g = to_global(c.pose, c.vcurr)
    vc, nc, vp, npv = (m.copy() for m in maps)
    pad_v, pad_n = np.full(W, np.nan, F), np.full(W, np.nan, F)
    pad_v[e["ux"]], vp[0, H - 1, e["ux"]], vp[1, H - 1, e["ux"]] = g
    pad_n[e["ux"]], npv[0, H - 1, e["ux"]], npv[1, H - 1, e["ux"]] = UP_N
    return pad_v, pad_n, [vc, nc, vp, npv]


def culling_margin_frames(W, H, x=9):
    """[(row, maps, rect)]: one vertex stored at pixel (x, row) whose projection is a tie half a pixel BEYOND its row -- row + 0.5 rounding up to row + 1
    and row - 0.5 rounding down to row - 1, for every odd row -- with the model's only normal at the pixel it rounds to.  Where `row` is the last
    (first) row of a workgroup's band of the batched pixel pass, the band's projected box ends exactly one pixel short of the model's rectangle:
    the margin the slab culling grows its boxes by is what keeps the inlier."""
    G = Geometry(W, H)
    out = []
    for row in range(1, H - 1, 2):
        for t in (row + 1, row - 1):
            v = _proj_vertex(G, float(x), (row + t) / 2.0)
            c = IcpCase(f"margin_{row}_{t}", IDENT, 1, False, [], v, UP_N, (x, t), v.copy(), UP_N)
            e = eval_icp(c, W, H, G.cx, G.cy)
            assert (e["ux"], e["uy"]) == (x, t) and float(e["py"]) == (row + t) / 2.0
            out.append((row, icp_frame(G, [c], [row * W + x]), np.array([x, t, x, t], np.int32)))
    return G, out
