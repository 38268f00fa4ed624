"""-m gpu: run culling and the in-place Model::clean on CRAFTED maps ("minefields").

A map of >= 6 M surfels (`bigMapElements`) lives as a sparse buffer of 512-slot runs; k_cull lists the runs that can be in view, k_cull_clean the
runs in which a rule of copy_unstable.vert:53-157 can apply, and only those are visited.  The claim "a run that is not listed holds no surfel whose
outcome the pass could change" is a conservativeness predicate: it is tested by inputs on its boundary.  The minefield is a natural room map
(synth.dense_room_map, > 256 runs, mostly out of view) with whole run-aligned blocks of 512 crafted surfels ("mines", plus a partial last run)
behind it, one block or more per class; a mine's box lies outside the view, so that only the rule it was built for can list its run:

  class            content                                                                   copy_unstable.vert says
  b-zero / b-neg   unstable, lastTime 0 resp. -5                                             dropped (:134, no rescue :136)
  b-minus1         lastTime -1, STABLE                                                        dropped
  b-minus2         lastTime -2                                                                kept, stamped with the tick (:131)
  b-recent         unstable, lastTime > 0, age reaches (20, timeDelta] during the run         dropped in that frame
  b-rescued        unstable, lastTime > 0, age > timeDelta                                    kept
  b-boundary       ages exactly 20, 21, timeDelta, timeDelta + 1 x confidence at / one ulp either side of the threshold   per > / < of the text
  nan-*            NaN position / confidence / lastTime, +-inf position                        whatever the oracle returns
  c-left/right/top/bottom/corner   in front of the camera, projecting outside that side: depth +-0.049 / +-0.051 m around the DEVICE's filtered
                   depth of the clamped border texel, which carries a foreign label           confidence x 0.25 (0.5 + 0.5 (1 - outlier / 10)) inside 5 cm
  c-plane-behind   -0.06 < z < -0.01, texel = a depth hole (filtered depth 0) with a foreign label   decays iff 0 is within 5 cm of z
  c-far-behind     z < -0.06, same texels                                                     untouched
  c-plane-front    0 < z < 0.06, same texels, stale (in view by the box test: no premise (i))  decays iff 0 is within 5 cm of z
  c-stale          in view, foreign label, age > timeDelta (k_cull drops the run, clean must visit it)   decays inside 5 cm
  a-edge           centres at u, v in {-2.5, -1.5, -0.5, 0, W, W + 0.5, W + 2.5} px, z at maxDepth +- 5 / 15 mm   index map / prediction per the oracle

The frames go through the FRAME-LEVEL path (stageFrame + fuseModels(0) + predictModels(0): enqueue_fusion_loop, the only caller of the culled clean)
in a multi-model context whose label image the test chooses, with a given pose (overridePose) and tick (setTick), timeDelta = 30, four frames
that carry mines across the 20-tick and timeDelta boundaries.  Like every -m gpu file this one also runs with MF_EMU=1 on the CPU-executed kernels."""
import os

import numpy as np
import pytest

from gpu_util import EMU

pytestmark = pytest.mark.gpu

TIME_DELTA = 30
CONF = 10.0             # the background's confidence threshold
T0 = 40                 # tick of the first frame
FRAMES = 4
DEPTH_CUT = 3.0
MAXD = 20.0             # maxDepthProcessed (mf_default_config)
OUTLIER = 0.9
RUN = 512
NEVER = 99

f32 = np.float32
KK = f32(0.5) + f32(0.5) * (f32(1) - f32(OUTLIER) / f32(10.0))
DECAY = f32(0.25) * KK       # copy_unstable.vert:150: a background surfel under a foreign object label


def _age_rule(L, conf, t):
    """copy_unstable.vert:128-136 restated (a surfel outside the image: the window rules :77-106 cannot apply): keep?"""
    L, conf, t = f32(L), f32(conf), f32(t)
    keep = True
    w = t if L == f32(-2) else L
    with np.errstate(invalid="ignore"):
        if w == f32(-1) or ((t - w) > 20 and conf < f32(CONF)):
            keep = False
        if w > 0 and t - w > f32(TIME_DELTA):
            keep = True
    return keep


def _scenario(W, H):
    from maskfusion_amd import synth
    f = 264.0 * W / 320.0
    st = synth.Stream(W=W, H=H, fx=f, fy=f, cx=W / 2.0, cy=H / 2.0, noise=False)
    rgb, depth, _ = st.frame(0)
    depth = np.array(depth, np.float32)
    mask = np.zeros((H, W), np.uint8)
    q = lambda a, n: int(round(a * n))
    reg = dict(left=(q(0.25, H), q(0.75, H)), right=(q(0.125, H), q(0.5, H)), top=(q(0.25, W), q(0.75, W)), bottom=(q(0.25, W), q(0.5, W)))
    mask[reg["left"][0]:reg["left"][1], 0] = 1
    mask[reg["left"][0]:reg["left"][0] + 8, 0] = 255             # maskValue < 255: an ignored texel decays nothing
    mask[reg["right"][0]:reg["right"][1], W - 1] = 2
    mask[0, reg["top"][0]:reg["top"][1]] = 1
    mask[0, reg["top"][0]:reg["top"][0] + 8] = 255
    mask[H - 1, reg["bottom"][0]:reg["bottom"][1]] = 3           # (H = 152: the bottom row lies in a partial 16 x 16 resolve tile)
    mask[0, 0] = 1
    mask[H - 1, W - 1] = 255
    patch = (q(0.25, H), q(0.25, H) + 12, q(0.3, W), q(0.3, W) + 16)      # interior, foreign label: c-stale
    mask[patch[0]:patch[1], patch[2]:patch[3]] = 1
    hole = (q(0.42, H), q(0.42, H) + 10, q(0.12, W), q(0.12, W) + 20)     # a depth hole with a foreign label: c-plane
    mask[hole[0]:hole[1], hole[2]:hole[3]] = 2
    depth[hole[0]:hole[1], hole[2]:hole[3]] = 0.0
    # the camera: a little off the map's origin, rotated by 2 deg (yaw) and 1 deg (pitch)
    a, b = np.deg2rad(2.0), np.deg2rad(1.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3] = Ry @ Rx
    T[:3, 3] = (0.05, -0.03, 0.10)
    T = T.astype(np.float32)
    return dict(W=W, H=H, f=f, cx=W / 2.0, cy=H / 2.0, st=st, rgb=rgb, depth=depth, mask=mask, T=T, reg=reg, patch=patch, hole=hole)


def _context(sc, **params):
    from maskfusion_amd import MaskFusion
    mf = MaskFusion(sc["W"], sc["H"], sc["f"], sc["f"], sc["cx"], sc["cy"], icpThresh=100.0, so3=False, enableMultipleModels=True, numGSurfels=1 << 18,
                    numOSurfels=1 << 12, initConfidenceGlobal=CONF, timeDelta=TIME_DELTA, depthCut=DEPTH_CUT, outlierCoefficient=OUTLIER)
    for k, v in params.items():
        mf.setParam(k, v)
    return mf


def _device_depthF(sc):
    mf = _context(sc)
    mf.stageFrame(sc["rgb"], sc["depth"], sc["mask"])
    d = mf.debugRead("depthF").copy()
    mf.close()
    return d


class _Field:
    """records + what the shader text says happens to every mine"""

    def __init__(self, sc, depthF, n_room=170_000, seed=7):
        from maskfusion_amd import synth
        self.sc, self.rng = sc, np.random.default_rng(seed)
        room = synth.dense_room_map(sc["st"].scene, n_room, last_time=float(T0 - 1), conf=20.0, zfront=-3.0)   # (a good part of it behind the camera)
        # in slabs of 0.25 m along z (creation order inside a slab): a run's box then lies in front of the camera plane or behind it, not across it --
        # with a foreign label anywhere in the frame, k_cull_clean has to list every run whose box straddles that plane
        room = room[np.argsort(np.floor(room[:, 2] / 0.25), kind="stable")]
        room = room[:(len(room) // RUN) * RUN]                   # the mines start on a run boundary
        self.n_room = len(room)
        self.parts, self.classes = [room], {}
        self.meta = []                                           # per mine: (class, texel x, texel y, delta / z, checked)
        self.depthF = depthF
        self._build()
        S = np.concatenate(self.parts).astype(np.float32)
        n_m = len(S) - self.n_room
        S[self.n_room:, 5] = np.arange(1, n_m + 1, dtype=np.float32)        # the record's unused word tags the mine
        self.S, self.n_mines = S, n_m
        assert self.n_room // RUN > 256 and n_m % RUN != 0        # several k_cull_clean workgroups; a partial last run

    # camera coordinates -> records in the map's frame
    def _records(self, pc, conf, L, name, checked=True, radius=0.004):
        sc = self.sc
        pc = np.asarray(pc, np.float64).reshape(-1, 3)
        n = len(pc)
        T = sc["T"].astype(np.float64)
        with np.errstate(invalid="ignore"):
            pw = pc @ T[:3, :3].T + T[:3, 3]
        pw[~np.isfinite(pc).all(1)] = pc[~np.isfinite(pc).all(1)]           # (a non-finite coordinate is uploaded as it is)
        rec = np.zeros((n, 12), np.float32)
        rec[:, :3] = pw
        rec[:, 3] = conf
        rec[:, 4] = float(0x808080)
        rec[:, 6] = 1.0
        rec[:, 7] = L
        rec[:, 8:11] = (T[:3, :3] @ np.array([0.0, 0.0, -1.0])).astype(np.float32)
        rec[:, 11] = radius
        at = sum(len(p) for p in self.parts) - self.n_room
        self.parts.append(rec)
        self.classes.setdefault(name, []).append((at, at + n, checked))
        return rec

    def _pixel(self, u, v, z):
        sc = self.sc
        u, v, z = (np.asarray(a, np.float64) for a in (u, v, z))
        return np.stack([(u - sc["cx"]) / sc["f"] * z, (v - sc["cy"]) / sc["f"] * z, z * np.ones_like(u)], -1)

    def _behind(self, n):
        r = self.rng
        return np.stack([r.uniform(-1, 1, n), r.uniform(-0.5, 0.5, n), r.uniform(-3.0, -1.0, n)], -1)

    def _front_outside(self, n):      # in front of the camera, far to the left of the image, nowhere near the depth of a border texel
        r = self.rng
        return self._pixel(r.uniform(-300, -150, n) * self.sc["W"] / 320.0, r.uniform(0, self.sc["H"], n), r.uniform(0.30, 0.40, n))

    def _build(self):
        sc, r, dF = self.sc, self.rng, self.depthF
        W, H = sc["W"], sc["H"]
        thr = f32(CONF)
        below, above = np.nextafter(thr, f32(0)), np.nextafter(thr, f32(100))
        self._records(self._behind(RUN), 1.0, 0.0, "b-zero")
        self._records(self._front_outside(RUN), 1.0, -5.0, "b-neg")
        self._records(self._behind(RUN), 20.0, -1.0, "b-minus1")
        self._records(self._behind(RUN), np.where(np.arange(RUN) % 2, 1.0, 20.0), -2.0, "b-minus2")
        # b-recent: age 21 in frame 0 / in frame 3 (lastTime 19 / 22)
        self._records(self._behind(RUN), 1.0, np.where(np.arange(RUN) % 2, 19.0, 22.0), "b-recent")
        self._records(self._front_outside(RUN), 1.0, 5.0, "b-rescued")
        Ls = np.array([T0 - 20, T0 - 21, T0 - TIME_DELTA, T0 - TIME_DELTA - 1], np.float32)
        cs = np.array([below, thr, above], np.float32)
        i = np.arange(RUN)
        self._records(self._behind(RUN), cs[i % 3], Ls[(i // 3) % 4], "b-boundary")
        # nan: one field at a time, on a stable stale base and on an unstable unstamped one; then two runs of NaN positions only
        for name, conf, L in (("nan-stable", 20.0, 5.0), ("nan-unstable", 1.0, 0.0)):
            rec = self._records(self._behind(RUN), conf, L, name, checked=False)
            k = np.arange(RUN) % 6
            rec[k == 0, 0] = np.nan
            rec[k == 1, 3] = np.nan
            rec[k == 2, 7] = np.nan
            rec[k == 3, 0] = np.inf
            rec[k == 4, 2] = -np.inf
        self._records(np.full((RUN, 3), np.nan), 1.0, 0.0, "nan-box-unstamped")            # dropped: rule (b) needs no box
        self._records(np.full((RUN, 3), np.nan), 1e5, float(T0 - 1), "nan-box-stable")       # kept, texel (0, 0): no comparison with NaN holds
        # c: the clamped border texel's filtered depth +- delta
        deltas = np.array([0.049, -0.049, 0.051, -0.051])
        far = lambda n, lo, hi: r.uniform(lo, hi, n)
        s = W / 320.0

        def border(name, tx, ty, u, v):
            z = dF[ty, tx].astype(np.float64) + deltas[np.arange(len(tx)) % 4]
            self._records(self._pixel(u, v, z), 1e5, float(T0 - 1), name)
            for a, b, d in zip(tx, ty, deltas[np.arange(len(tx)) % 4]):
                self.meta.append((name, int(a), int(b), float(d)))
        n = RUN
        rows = lambda lo, hi: lo + (np.arange(n) // 4) % (hi - lo)
        ty = rows(*sc["reg"]["left"]); border("c-left", np.zeros(n, int), ty, far(n, -250 * s, -120 * s), ty + 0.5)
        ty = rows(*sc["reg"]["right"]); border("c-right", np.full(n, W - 1), ty, far(n, W + 120 * s, W + 250 * s), ty + 0.5)
        tx = rows(*sc["reg"]["top"]); border("c-top", tx, np.zeros(n, int), tx + 0.5, far(n, -200 * s, -100 * s))
        tx = rows(*sc["reg"]["bottom"]); border("c-bottom", tx, np.full(n, H - 1), tx + 0.5, far(n, H + 100 * s, H + 200 * s))
        border("c-corner", np.zeros(n, int), np.zeros(n, int), far(n, -250 * s, -120 * s), far(n, -200 * s, -100 * s))
        # c-plane: texels of the depth hole
        h0, h1, w0, w1 = sc["hole"]
        ys, xs = np.nonzero((dF[h0:h1, w0:w1] == 0) & (sc["mask"][h0:h1, w0:w1] == 2))
        assert len(ys) >= 50, "the depth hole did not survive the filter"
        pick = np.arange(n) % len(ys)
        hx, hy = xs[pick] + w0, ys[pick] + h0

        def plane(name, zs, L):
            z = np.asarray(zs)[np.arange(n) % len(zs)]
            self._records(self._pixel(hx + 0.5, hy + 0.5, z), 1e5, L, name)
            for a, b, d in zip(hx, hy, z):
                self.meta.append((name, int(a), int(b), float(d)))
        plane("c-plane-behind", [-0.058, -0.04, -0.02, -0.012], float(T0 - 1))
        plane("c-far-behind", [-0.07, -0.2, -1.0], float(T0 - 1))
        plane("c-plane-front", [0.012, 0.03, 0.049, 0.051], 5.0)
        # c-stale: pixel centres of the interior patch
        p0, p1, q0, q1 = sc["patch"]
        px, py = q0 + np.arange(n) % (q1 - q0), p0 + (np.arange(n) // (q1 - q0)) % (p1 - p0)
        z = dF[py, px].astype(np.float64) + deltas[np.arange(n) % 4]
        self._records(self._pixel(px + 0.5, py + 0.5, z), 1e5, 5.0, "c-stale")
        for a, b, d in zip(px, py, deltas[np.arange(n) % 4]):
            self.meta.append(("c-stale", int(a), int(b), float(d)))
        # a-edge (a partial last run): the image's edges and the far limit of the projection passes
        e = np.array([-2.5, -1.5, -0.5, 0.0, W, W + 0.5, W + 2.5])
        eh = np.array([-2.5, -1.5, -0.5, 0.0, H, H + 0.5, H + 2.5])
        pts = [self._pixel(u, H / 2.0 + 0.5, z) for u in e for z in (1.0, 2.0)] + [self._pixel(W / 2.0 + 0.5, v, z) for v in eh for z in (1.0, 2.0)]
        pts += [self._pixel(W / 2.0 + 8.5 + 2 * j, H / 2.0 + 0.5, MAXD + d) for j, d in enumerate((-0.015, -0.005, 0.005, 0.015))]
        pts += [self._pixel(u, v, z) for u in (0.0, W / 2.0, float(W)) for v in (0.0, float(H)) for z in (-0.02, 0.02)]
        pts += [np.array([x, 0.0, z]) for x in (-0.01, 0.01) for z in (-0.02, 0.0, 0.02)]           # a box that straddles the near plane
        self._records(np.stack(pts), 20.0, float(T0 - 1), "a-edge", checked=False)

    # ---- what the text says ------------------------------------------------------------------------------------------------------------------
    def intent(self):
        """per mine: frame in which it is dropped (NEVER: none), whether it decays in every frame, whether it is asserted at all"""
        S = self.S[self.n_room:]
        n = self.n_mines
        drop_at, decays, checked, stamped = np.full(n, NEVER), np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
        for name, blocks in self.classes.items():
            for a, b, chk in blocks:
                checked[a:b] = chk
                if name.startswith("nan-box"):
                    checked[a:b] = True
                if name.startswith("b-") or name.startswith("nan-box"):
                    for i in range(a, b):
                        for k in range(FRAMES):
                            if not _age_rule(S[i, 7], S[i, 3], T0 + k):
                                drop_at[i] = k
                                break
                if name == "b-minus2":
                    stamped[a:b] = True
        at = {}
        for name, blocks in self.classes.items():
            at[name] = blocks[0][0]
        seen = {}
        mask, dF = self.sc["mask"], self.depthF
        for (name, tx, ty, d) in self.meta:
            i = at[name] + seen.get(name, 0)
            seen[name] = seen.get(name, 0) + 1
            foreign = mask[ty, tx] != 0 and mask[ty, tx] < 255
            if name.startswith("c-plane") or name == "c-far-behind":
                z = f32(d)        # the texel's filtered depth is 0: `0 > z - 0.05 && 0 < z + 0.05`
                decays[i] = foreign and (f32(0) > z - f32(0.05)) and (f32(0) < z + f32(0.05))
            else:
                decays[i] = foreign and abs(d) < 0.05 and dF[ty, tx] == dF[ty, tx]
        return drop_at, decays, checked, stamped

    def blocks(self):
        return [(name, a, b) for name, bl in self.classes.items() for a, b, _ in bl]


def _box_outside_view(sc, rec):
    """premise (i), host fp64: every corner of the records' box (in the map's frame, as the run table keeps it) outside the SAME side of the image
    grown by 2 px, or behind the near plane -- a cull by the view alone skips the run"""
    p = rec[:, :3].astype(np.float64)
    p = p[np.isfinite(p).all(1)]
    if len(p) == 0:
        return True
    lo, hi = p.min(0), p.max(0)
    Ti = np.linalg.inv(sc["T"].astype(np.float64))
    c = np.array([[(hi if i & 1 else lo)[0], (hi if i & 2 else lo)[1], (hi if i & 4 else lo)[2]] for i in range(8)])
    h = c @ Ti[:3, :3].T + Ti[:3, 3]
    f, cx, cy, W, H = sc["f"], sc["cx"], sc["cy"], sc["W"], sc["H"]
    x, y, z = h[:, 0], h[:, 1], h[:, 2]
    return bool((z < -0.01).all() or (f * x + (cx + 2) * z < 0).all() or (f * x + (cx - W - 2) * z > 0).all() or (f * y + (cy + 2) * z < 0).all() or
                (f * y + (cy - H - 2) * z > 0).all())


FORMS = {
    "culled": dict(bigMapElements=0, cullRuns=1),
    "unculled": dict(bigMapElements=0, cullRuns=0),
    "small": dict(bigMapElements=1 << 30, inPlaceElements=1 << 30),
    "densify": dict(bigMapElements=0, cullRuns=1, densifyEvery=1),
}


def _run(sc, S, params, download=True, frames=FRAMES):
    """four frames through the frame-level path.  download: the map after every frame (a download compacts a sparse buffer: the next frame starts from
    a fresh table); without it the buffer stays sparse over the whole run and only the last frame's map is read"""
    mf = _context(sc, **params)
    bg = mf.getBackgroundModel()
    mf.stageFrame(sc["rgb"], sc["depth"], sc["mask"])
    bg.uploadMap(S)
    bg.overridePose(sc["T"]); bg.overridePose(sc["T"])
    mf.setTick(T0)
    out = []
    for k in range(frames):
        if k > 0:
            mf.stageFrame(sc["rgb"], sc["depth"], sc["mask"])
        mf.fuseModels(0)
        stats = dict(clean=mf.getParam("cleanRuns"), runs=mf.getParam("backgroundRuns"), densify=mf.getParam("densifyCount"),
                     unstamped=mf.getParam("unstampedRuns"))
        cand = dict(op=mf.debugRead("cand_op", count=((sc["W"] + 1) // 2) * ((sc["H"] + 1) // 2)).copy()) if download else {}
        mf.predictModels(0, k)
        o = dict(count=bg.lastCount(), pose=bg.getPose(), index=mf.debugRead("index").copy(), pv=bg.debugRead("pred_vertex").copy(),
                 pi=bg.debugRead("pred_image").copy(), pt=bg.debugRead("pred_time").copy(), pn=bg.debugRead("pred_normal").copy(), tick=mf.getTick(), **stats, **cand)
        if download or k == frames - 1:
            o["map"] = bg.downloadMap().copy()
        out.append(o)
    mf.close()
    return out


@pytest.fixture(scope="module", params=[(320, 240), (200, 152)], ids=["320x240", "200x152"])
def field(request, hip):
    sc = _scenario(*request.param)
    fld = _Field(sc, _device_depthF(sc))
    cache = {}

    def run(name, download=True):
        key = (name, download)
        if key not in cache:
            cache[key] = _run(sc, fld.S, FORMS[name], download)
        return cache[key]
    return dict(sc=sc, fld=fld, run=run)


def _mines(fld, cloud):
    """cloud (a downloaded map) -> per mine: row in the cloud or -1"""
    tag = cloud[:, 5]
    rows = np.full(fld.n_mines + 1, -1)
    live = np.nonzero((tag >= 1) & (tag <= fld.n_mines))[0]
    rows[tag[live].astype(np.int64)] = live
    assert len(np.unique(tag[live])) == len(live)
    return rows[1:]


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), what


def test_premises_box_and_culling(field):
    """(i) every mine block's box is outside the image grown by 2 px (c-stale, c-plane-front and a-edge excepted: in or at the view by design);
    (ii) the culled clean visits fewer than 0.7 of the runs in every frame."""
    sc, fld = field["sc"], field["fld"]
    bad = []
    for name, a, b in fld.blocks():
        if name in ("c-stale", "c-plane-front", "a-edge"):
            continue
        if not _box_outside_view(sc, fld.S[fld.n_room + a:fld.n_room + b]):
            bad.append(name)
    print("premise (i): mine blocks whose box reaches into the view:", bad, "of", len(fld.blocks()))
    assert not bad
    for k, o in enumerate(field["run"]("culled", download=False)):
        print(f"premise (ii): frame {k}: clean visited {o['clean']:.0f} of {o['runs']:.0f} runs, compactions so far {o['densify']:.0f}")
        assert 0 < o["clean"] < 0.7 * o["runs"] and o["runs"] > 256
        assert o["densify"] == 0          # the buffer stayed sparse over the run
        # the table's "holds a time stamp <= 0" bit: behind the first clean only the runs whose unstamped surfels are KEPT still carry it -- the
        # stable halves of nan-unstable's block (lastTime 0, NaN confidence) and nothing else (b-minus2 is stamped with the tick by then)
        print(f"             runs that carry a time stamp <= 0 behind the frame: {o['unstamped']:.0f}")
        assert o["unstamped"] == 1


def test_forms_agree_on_the_minefield(field):
    """culled in place == unculled in place == small forms == in place with a compaction before every frame: count, pose, map (NaN-aware), index
    map and prediction taps, on every frame -- with the map read after every frame, and with a buffer that stays sparse over all four frames."""
    ref = field["run"]("small")
    for name, download in (("culled", True), ("culled", False), ("unculled", True), ("unculled", False), ("densify", True)):
        got = field["run"](name, download)
        for k, (x, y) in enumerate(zip(ref, got)):
            what = (name, "download" if download else "sparse", "frame", k)
            assert x["count"] == y["count"] and x["tick"] == y["tick"], what + (x["count"], y["count"])
            assert np.array_equal(x["pose"], y["pose"]), what
            for tap in ("pv", "pn", "pi", "pt"):
                _same(x[tap], y[tap], what + (tap,))
            # the index map holds SLOTS: the same numbers where the frame started from a dense buffer (every frame behind a download, the first
            # frame of any run), the same texels filled where the buffer has become sparse
            if download or k == 0:
                _same(x["index"], y["index"], what + ("index",))
            else:
                _same(x["index"] > 0, y["index"] > 0, what + ("index > 0",))
            if "map" in y:
                if not (x["map"].shape == y["map"].shape and np.array_equal(x["map"], y["map"], equal_nan=True)):
                    fld = field["fld"]
                    ra, rb = _mines(fld, x["map"]), _mines(fld, y["map"])
                    diff = {n: int(((ra[a:b] >= 0) != (rb[a:b] >= 0)).sum()) for n, a, b in fld.blocks()}
                    pytest.fail(f"{what}: maps differ; surfels {len(x['map'])} vs {len(y['map'])}; mines kept on one side only, per class: "
                                f"{ {n: v for n, v in diff.items() if v} }")


def _expected_conf(conf0, n_decays):
    c = f32(conf0)
    for _ in range(n_decays):
        c = f32(c * DECAY)
    return c


def _check_classes(fld, maps, who):
    """the per-class outcomes of the table, from the shader text alone; maps: the map after every frame.  Returns the share of mines per class whose
    outcome is the intended one (asserted by the caller)."""
    drop_at, decays, checked, stamped = fld.intent()
    S = fld.S[fld.n_room:]
    share = {}
    for name, a, b in fld.blocks():
        ok = np.ones(b - a, bool)
        for k, cloud in enumerate(maps):
            rows = _mines(fld, cloud)[a:b]
            alive = rows >= 0
            ok &= alive == (drop_at[a:b] > k)
            for j in np.nonzero(alive & ok)[0]:
                i = a + j
                want = _expected_conf(S[i, 3], k + 1) if decays[i] else S[i, 3]
                got = cloud[rows[j], 3]
                ok[j] &= bool(got == want) or bool(np.isnan(got) and np.isnan(want))
                if stamped[i]:
                    ok[j] &= cloud[rows[j], 7] == T0      # stamped with the tick of the first pass that met it
        share.setdefault(name, []).append(float(ok.mean()))
    print(f"{who}: share of mines with the intended outcome over {len(maps)} frames, per class:")
    for name, v in share.items():
        n_dec = int(sum(decays[a:b].sum() for nm, a, b in fld.blocks() if nm == name))
        n_drop = int(sum((drop_at[a:b] < NEVER).sum() for nm, a, b in fld.blocks() if nm == name))
        print(f"   {name:18s} {min(v):.3f}   (mines meant to decay {n_dec}, to be dropped {n_drop})")
    return {k: min(v) for k, v in share.items()}, checked


ORACLE_ONLY = ("nan-stable", "nan-unstable", "a-edge")


def _oracle_frame(mfo, sc, depthF, S_pre, tick, cap):
    cam = mfo.cam(sc["W"], sc["H"], sc["f"], sc["f"], sc["cx"], sc["cy"])
    T, n = sc["T"], len(S_pre)
    wgt = mfo.fusion_weight(T, T, 1.0)
    idx, vc, ct, nr = mfo.predict_indices(cam, T, S_pre, n, tick, MAXD, TIME_DELTA)
    op, best, rec = mfo.fuse_data(cam, T, sc["rgb"], sc["depth"], depthF, sc["mask"], 0, tick, wgt, DEPTH_CUT, idx, vc, nr)
    S2 = mfo.fuse_update(S_pre, n, tick, op, best, rec)
    idx2, vc2, ct2, nr2 = mfo.predict_indices(cam, T, S2, n, tick, MAXD, TIME_DELTA)
    S3, n3 = mfo.clean(cam, T, S2, n, op, rec, tick, TIME_DELTA, CONF, MAXD, OUTLIER, 0, idx2, vc2, ct2, nr2, depthF, sc["mask"], cap)
    pred = mfo.combined_predict(cam, T, S3, n3, MAXD, CONF, tick, tick, TIME_DELTA)
    return S3, n3, idx, pred, op


def test_oracle_premise_every_class_tests_something(field, oracle):
    """premise (iii): the ORACLE's outcome is the intended one for >= 90 % of the mines of every c-class and for all of the others -- a class that
    silently tests nothing fails.  The oracle alone, chained over the four frames on its own maps, fed the device's filtered depth."""
    sc, fld = field["sc"], field["fld"]
    S, maps = fld.S, []
    for k in range(FRAMES):
        S, n, _, _, _ = _oracle_frame(oracle, sc, fld.depthF, S, T0 + k, 1 << 18)
        maps.append(S)
    share, _ = _check_classes(fld, maps, "oracle")
    for name, v in share.items():
        if name in ORACLE_ONLY:
            continue
        assert v >= (0.9 if name.startswith("c-") else 1.0), (name, v)
    drop_at, decays, _, _ = fld.intent()
    for name, a, b in fld.blocks():       # every class does what its name says for a good part of its mines
        if name.startswith("c-") and name != "c-far-behind":
            assert 0.25 <= decays[a:b].mean() <= 0.8, (name, decays[a:b].mean())
        if name in ("b-zero", "b-neg", "b-minus1", "b-recent", "nan-box-unstamped"):
            assert (drop_at[a:b] < NEVER).all(), name
        if name in ("b-rescued", "b-minus2", "c-far-behind", "nan-box-stable"):
            assert (drop_at[a:b] == NEVER).all() and not decays[a:b].any(), name
    a, b = fld.classes["b-boundary"][0][:2]
    assert 0.2 < (drop_at[a:b] < NEVER).mean() < 0.8


def test_culled_clean_does_what_the_shader_text_says(field):
    """per class, independent of the oracle: dropped / kept in the right frame, decayed by exactly the factor (fp32), a -2 stamp replaced by the tick --
    on the culled frame-level path with a buffer that is read after every frame, and on the final map of the run that stayed sparse."""
    fld = field["fld"]
    share, _ = _check_classes(fld, [o["map"] for o in field["run"]("culled")], "culled in place")
    for name, v in share.items():
        if name not in ORACLE_ONLY:
            assert v == 1.0, (name, v)
    # the run without downloads: the last map alone
    last = field["run"]("culled", download=False)[-1]["map"]
    drop_at, decays, checked, _ = fld.intent()
    rows = _mines(fld, last)
    S = fld.S[fld.n_room:]
    for name, a, b in fld.blocks():
        if name in ORACLE_ONLY:
            continue
        assert np.array_equal(rows[a:b] >= 0, drop_at[a:b] == NEVER), name
        for i in range(a, b):
            if rows[i] >= 0:
                want = _expected_conf(S[i, 3], FRAMES) if decays[i] else S[i, 3]
                assert last[rows[i], 3] == want or (np.isnan(want) and np.isnan(last[rows[i], 3])), (name, i, last[rows[i], 3], want)


def _close(a, b, tol, what):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    fin = np.isfinite(b)
    assert np.array_equal(fin, np.isfinite(a)) and np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: non-finite pattern differs"
    assert np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]), f"{what}: infinities differ"
    err = np.abs(a[fin] - b[fin])
    bad = err > tol * np.maximum(1.0, np.abs(b[fin]))
    print(f"  {what}: {int((err > 0).sum())} of {err.size} not bit-identical, max err {err.max() if err.size else 0.0:.3g}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {err.size} beyond {tol}, max err {err.max()}"


def test_culled_frame_level_path_against_oracle(field, oracle):
    """the chain of test_gpu_surfel_passes.py::test_surfel_passes_against_oracle (predict_indices -> fuse_data -> fuse_update -> predict_indices ->
    clean -> combined_predict, the oracle fed the device's filtered depth and the same label image, maskID 0) against the CULLED FRAME-LEVEL path,
    frame by frame from the device's own map before the frame: survivor count exact, keep / drop per mine exact, colour and stamps exact,
    position / confidence / normal 1e-6 (PARITY.md 2c)."""
    sc, fld = field["sc"], field["fld"]
    S_pre = fld.S
    for k, o in enumerate(field["run"]("culled")):
        S3, n3, idx, (img, pv, pn, ptime), op = _oracle_frame(oracle, sc, fld.depthF, S_pre, T0 + k, 1 << 18)
        g = o["map"]
        print(f"frame {k}: in {len(S_pre)} -> oracle {n3}, device {len(g)}; candidate op flips {int((op != o['op'][:len(op)]).sum())}")
        assert np.array_equal(o["index"], idx), k
        assert len(g) == n3, (k, len(g), n3)
        ra, rb = _mines(fld, g), _mines(fld, S3)
        assert np.array_equal(ra >= 0, rb >= 0), (k, int(((ra >= 0) != (rb >= 0)).sum()))
        assert np.array_equal(ra, rb), k                                  # every mine in the same slot
        _close(g[:, :4], S3[:, :4], 1e-6, f"frame {k}: position / confidence")
        assert np.array_equal(g[:, 4:8], S3[:, 4:8], equal_nan=True), k    # colour, tag, stamps
        ok = np.isfinite(S3[:, 8:]).all(1)
        _close(g[ok][:, 8:], S3[ok][:, 8:], 1e-6, f"frame {k}: normal / radius")
        assert np.array_equal(o["pi"], img) and np.array_equal(o["pt"], ptime), k
        _close(o["pv"], pv, 1e-6, f"frame {k}: predicted vertex / confidence")
        S_pre = g


# ------------------------------------------------------------------------------------------------------------------------------------------------
# every entry point that reads or writes a model's buffer, on a SPARSE buffer: the same call on a context in place (sparse, with holes) and on one in
# the small forms (dense) -- equal outputs, and the next two frames bit-identical
# ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field152(hip):
    sc = _scenario(200, 152)
    return dict(sc=sc, fld=_Field(sc, _device_depthF(sc)))


def _frame(mf, sc, k):
    mf.stageFrame(sc["rgb"], sc["depth"], sc["mask"])
    mf.fuseModels(0)
    mf.predictModels(0, k)


def _taps(mf):
    bg = mf.getBackgroundModel()
    return dict(count=bg.lastCount(), tick=mf.getTick(), pv=bg.debugRead("pred_vertex").copy(), pn=bg.debugRead("pred_normal").copy(),
                pi=bg.debugRead("pred_image").copy(), pt=bg.debugRead("pred_time").copy())


def _pair(sc, S):
    out = []
    for params in (FORMS["culled"], FORMS["small"]):
        mf = _context(sc, **params)
        bg = mf.getBackgroundModel()
        mf.stageFrame(sc["rgb"], sc["depth"], sc["mask"])
        bg.uploadMap(S)
        bg.overridePose(sc["T"]); bg.overridePose(sc["T"])
        mf.setTick(T0)
        mf.fuseModels(0)
        mf.predictModels(0, 0)
        _frame(mf, sc, 1)
        out.append(mf)
    return out


def _assert_sparse(mf):
    """the in-place context's buffer is sparse (a run table, holes: whole blocks of mines have died) and has not been compacted"""
    assert mf.getParam("backgroundRuns") > 0 and mf.getParam("densifyCount") == 0


def _two_more_frames_agree(a, b, sc, what, first=2):
    for k in range(first, first + 2):
        _frame(a, sc, k); _frame(b, sc, k)
        x, y = _taps(a), _taps(b)
        assert x["count"] == y["count"] and x["tick"] == y["tick"], (what, k, x["count"], y["count"])
        for tap in ("pv", "pn", "pi", "pt"):
            _same(x[tap], y[tap], (what, k, tap))
    ca, cb = a.getBackgroundModel().downloadMap(), b.getBackgroundModel().downloadMap()
    assert ca.shape == cb.shape and np.array_equal(ca, cb, equal_nan=True), what


def _call_rebuild(mf, fld, tmp):
    mf.setParam("rebuildRunTable", 1)
    return mf.getBackgroundModel().lastCount()


def _call_upload(mf, fld, tmp):
    S = fld.S[RUN * 40:].copy()             # another map: replaces the sparse buffer
    mf.getBackgroundModel().uploadMap(S)
    return mf.getBackgroundModel().lastCount()


def _call_set_tick(mf, fld, tmp):
    mf.setTick(T0 + 19)                     # b-recent / b-boundary survivors cross the 20-tick boundary at once, stale ones timeDelta
    return mf.getTick()


def _call_model_passes(mf, fld, tmp):
    bg, t = mf.getBackgroundModel(), mf.getTick()
    mf.stageFrame(fld.sc["rgb"], fld.sc["depth"], fld.sc["mask"])
    bg.predictIndices(t, MAXD, TIME_DELTA)
    filled = mf.debugRead("index") > 0
    bg.fuse(t, DEPTH_CUT, 1.0)
    bg.predictIndices(t, MAXD, TIME_DELTA)
    bg.clean(t, TIME_DELTA, MAXD)
    bg.combinedPredict(MAXD, t, t, TIME_DELTA)
    mf.endFrame(7)
    tp = _taps(mf)
    return [filled, tp["count"], tp["pv"], tp["pn"], tp["pi"], tp["pt"]]


def _call_download(mf, fld, tmp):
    return mf.getBackgroundModel().downloadMap()


def _call_save_ply(mf, fld, tmp):
    d = os.path.join(tmp, f"ply{len(os.listdir(tmp))}")
    os.makedirs(d)
    mf.savePly(d + os.sep)
    files = sorted(os.listdir(d))
    assert files, "savePly wrote nothing"
    return [files] + [np.frombuffer(open(os.path.join(d, f), "rb").read(), np.uint8) for f in files]


def _render_views(mf, sc):
    """the camera's follow view, and a view turned round to where the mines behind the camera lie, unstable surfels drawn as points: the emptied runs
    there still hold the records of the mines that died, which only a render that read dead slots would draw"""
    from maskfusion_amd import synth
    v = mf.defaultRenderView(sc["W"], sc["H"])
    v.fx = v.fy = sc["f"]
    v.background_color_type = 2
    b = mf.defaultRenderView(sc["W"], sc["H"])
    b.fx = b.fy = sc["f"]
    b.background_color_type, b.draw_unstable, b.draw_points = 1, 1, 1
    b.set_pose(v.pose() @ synth.make_pose(synth.rot_xyz(0.0, np.pi, 0.0), [0.0, 0.0, 0.0]))
    return [("follow", v), ("turned round, unstable points", b)]


def _call_render(mf, fld, tmp):
    """the headless render reads the run table itself (mf_render.hip): both views on the sparse buffer first (the outputs the two contexts must
    agree on bit for bit), then against the numpy restatement (whose download compacts the buffer) as tests/test_gpu_render.py::
    test_render_agrees_with_restatement does: colour, model and depth exact / 1e-5 wherever the restatement is not ambiguous.  That test's bound on the
    NUMBER of ambiguous pixels (0.5 %) is a property of its scene and is not taken over: this map's walls are exact planes of overlapping discs,
    so the two nearest discs tie within 2e-6 at most pixels; there the depth is compared all the same (a tie has one depth)."""
    import render_restatement as rr
    sc = fld.sc
    n0 = mf.getParam("densifyCount")
    views = _render_views(mf, sc)
    outs = [mf.renderView(v, depth=True, models=True) for _, v in views]
    assert mf.getParam("densifyCount") == n0          # the render changes nothing
    for (name, v), (rgba, dep, mod) in zip(views, outs):
        r_rgba, r_dep, r_mod, amb = rr.render(mf, v, None, time_delta=TIME_DELTA)
        ok = ~amb
        drawn = r_mod >= 0
        cdiff = np.abs(rgba.astype(int) - r_rgba.astype(int)).max(2)
        rel = np.abs(dep[drawn] - r_dep[drawn]) / np.maximum(np.abs(r_dep[drawn]), 1e-30)
        print(f"render, {name}: drawn {int(drawn.sum())}, of them unambiguous {int((drawn & ok).sum())}, colour mismatches {int(((cdiff > 1) & ok).sum())}, "
              f"model mismatches {int(((mod != r_mod) & ok).sum())}, max depth rel {rel.max() if rel.size else 0:.3g}")
        assert drawn.sum() > 0.05 * v.width * v.height and (drawn & ok).sum() > 100, name
        assert int(((mod != r_mod) & ok).sum()) == 0 and int(((cdiff > 1) & ok).sum()) == 0, name
        assert np.array_equal(mod >= 0, drawn) or int((((mod >= 0) != drawn) & ok).sum()) == 0, name
        assert rel.max() <= 1e-5 + 2e-6, name          # (ambiguous pixels included: the restatement's tie margin on top of the depth gate)
        assert (dep[ok & ~drawn] == 0).all(), name
    return [a for out in outs for a in out]


def _call_exports(mf, fld, tmp):
    """the -el / -en / -ev exports of the command line (cli.export_renders) after the frame just processed"""
    from maskfusion_amd import cli
    d = os.path.join(tmp, f"exp{len(os.listdir(tmp))}")
    os.makedirs(d)
    n0 = mf.getParam("densifyCount")
    cli.export_renders(mf, {"-el": "1", "-en": "1", "-ev": "1"}, d + os.sep)
    assert mf.getParam("densifyCount") == n0
    files = sorted(os.listdir(d))
    assert len(files) == 3, files
    from PIL import Image
    imgs = [np.asarray(Image.open(os.path.join(d, f))) for f in files]
    assert all((im != im[0, 0]).any() for im in imgs), "an export drew nothing"
    return [files] + imgs


CALLS = dict(renderView=_call_render, exports=_call_exports, rebuildRunTable=_call_rebuild, uploadMap=_call_upload, setTick=_call_set_tick, modelPasses=_call_model_passes, downloadMap=_call_download,
             savePly=_call_save_ply)


@pytest.mark.parametrize("call", list(CALLS))
def test_entry_points_on_a_sparse_buffer(field152, call, tmp_path):
    sc, fld = field152["sc"], field152["fld"]
    a, b = _pair(sc, fld.S)
    _assert_sparse(a)
    ra, rb = CALLS[call](a, fld, str(tmp_path)), CALLS[call](b, fld, str(tmp_path))
    ra, rb = (ra if isinstance(ra, list) else [ra]), (rb if isinstance(rb, list) else [rb])
    assert len(ra) == len(rb)
    for i, (x, y) in enumerate(zip(ra, rb)):
        if isinstance(x, np.ndarray):
            _same(x, y, (call, "output", i))
        else:
            assert x == y, (call, "output", i, x, y)
    _two_more_frames_agree(a, b, sc, call)
    a.close(); b.close()


def test_model_cloud_nn_on_a_sparse_map_of_more_than_1024_runs(hip):
    """k_run_offsets scans the run table in chunks of 1024 runs with a carry: a sparse map of > 1024 runs (>= 600 k live surfels) with EMPTIED runs among
    them (every 9th run of the uploaded map dies in the first frame), against ev.nearest on the download with the same NaN filter, bit for bit."""
    from maskfusion_amd import eval as ev, synth
    sc = _scenario(200, 152)
    room = synth.dense_room_map(sc["st"].scene, 720_000, last_time=float(T0 - 1), conf=20.0, zfront=-3.0)
    room = room[:(len(room) // RUN) * RUN]
    runs = len(room) // RUN
    dead = (np.arange(len(room)) // RUN) % 9 == 4
    room[dead, 3] = 1.0
    room[dead, 7] = 0.0                    # unstable, never stamped: dropped by the age rule wherever the run lies
    from maskfusion_amd import MaskFusion
    mf = MaskFusion(sc["W"], sc["H"], sc["f"], sc["f"], sc["cx"], sc["cy"], icpThresh=100.0, so3=False, enableMultipleModels=True, numGSurfels=1 << 20,
                    numOSurfels=1 << 12, initConfidenceGlobal=CONF, timeDelta=TIME_DELTA, depthCut=DEPTH_CUT, outlierCoefficient=OUTLIER)
    mf.setParam("bigMapElements", 0)
    bg = mf.getBackgroundModel()
    mf.stageFrame(sc["rgb"], sc["depth"], sc["mask"])
    bg.uploadMap(room)
    bg.overridePose(sc["T"]); bg.overridePose(sc["T"])
    mf.setTick(T0)
    mf.fuseModels(0); mf.predictModels(0, 0)
    _frame(mf, sc, 1)
    n = bg.lastCount()
    print("runs", mf.getParam("backgroundRuns"), "surfels", n, "of", len(room), "uploaded; emptied runs", int(dead.sum()) // RUN)
    assert mf.getParam("backgroundRuns") > 1024 and runs > 1024 and n >= 600_000 and mf.getParam("densifyCount") == 0
    assert n < len(room) - int(dead.sum()) + 40_000          # the dead runs are gone
    rng = np.random.default_rng(3)
    q = rng.uniform([-2.4, -1.4, -2.9], [2.4, 1.1, 2.7], (4000, 3)).astype(np.float32)
    q[::2] = room[rng.integers(0, len(room), 2000), :3] + rng.normal(0, 0.01, (2000, 3)).astype(np.float32)
    thr = bg.getConfidenceThreshold()
    got = {name: mf.modelCloudNN(0, q, 0.05, confThreshold=ct) for name, ct in (("own threshold", None), ("all", -1.0))}
    assert mf.getParam("densifyCount") == 0                  # the query left the map as it was
    surf = bg.downloadMap()
    assert len(surf) == n
    for name, ct in (("own threshold", thr), ("all", -1.0)):
        tgt = surf.copy()
        tgt[~(surf[:, 3] > ct), :3] = np.nan
        d, i = ev.nearest(tgt, q, 0.05)
        assert (got[name][1] >= 0).mean() > 0.3, name
        assert got[name][0].tobytes() == d.tobytes(), name
        assert np.array_equal(got[name][1], i), name
    mf.close()


@pytest.mark.skipif(EMU, reason="event timings need the GPU")
def test_pass_timings_report_the_last_frame_only(hip):
    """`passTimings`: "compaction ... 0 in a frame without one" (include/maskfusion_amd.h) -- a frame that compacts, then one that does not; likewise
    bgAppend when the frame takes the two-launch form and objFuseClean without object models.  Only the 0 / non-0 pattern is asserted."""
    from maskfusion_amd import MaskFusion, synth
    W, H, f = 320, 240, 264.0
    st = synth.Stream(W=W, H=H, fx=f, fy=f, cx=W / 2.0, cy=H / 2.0, noise=True)
    frames = [st.frame(k) for k in range(6)]
    mf = MaskFusion(W, H, f, f, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, enableMultipleModels=False, numGSurfels=1 << 19, initConfidenceGlobal=10.0)
    mf.setParam("bigMapElements", 0)
    mf.setParam("passTimings", 1)
    seen = []
    for k, (rgb, d, _) in enumerate(frames):
        if k == 3:
            mf.setParam("densifyEvery", 1)         # this frame compacts the (sparse) buffer ...
        if k == 4:
            mf.setParam("densifyEvery", 0)         # ... this one does not
        if k == 5:
            mf.setParam("bigMapElements", 1 << 30)  # the two-launch clean: no append pass (and a compaction on the way back to a dense buffer)
        n0 = mf.getParam("densifyCount")
        mf.processFrame(rgb, d, timestamp=k)
        t = mf.passTimings()
        seen.append((mf.getParam("densifyCount") - n0, t))
        print(k, "compactions", seen[-1][0], {key: round(v, 4) for key, v in t.items() if v})
    assert "compaction" in seen[0][1] and "bgAppend" in seen[0][1] and "objFuseClean" in seen[0][1], list(seen[0][1])
    assert seen[3][0] == 1 and seen[3][1]["compaction"] > 0 and seen[3][1]["bgAppend"] > 0
    assert seen[4][0] == 0 and seen[4][1]["compaction"] == 0 and seen[4][1]["bgAppend"] > 0
    assert seen[5][1]["bgAppend"] == 0 and seen[5][1]["bgClean"] > 0
    assert all(t["objFuseClean"] == 0 for _, t in seen)        # (a single-model context)
    mf.close()
    # objFuseClean: frames whose object models go through the batched passes, then a frame that handles them one by one (the pass does not run)
    st = synth.Stream(W=W, H=H, fx=f, fy=f, cx=W / 2.0, cy=H / 2.0, noise=True, n_objects=3, object_motion=0.0)
    mf = MaskFusion(W, H, f, f, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, enableMultipleModels=True, numGSurfels=1 << 19, numOSurfels=1 << 16,
                    modelSpawnOffset=2, trackAllModels=False, initConfidenceGlobal=10.0, initConfidenceObject=0.01)
    for k, v in (("mfThreshold", 0.3), ("mfWeightDistance", 150.0), ("mfWeightConvexity", 2.8), ("mfMorphEdgeIterations", 0),
                 ("mfMorphMaskIterations", 0), ("newModelMinRelativeSize", 0.004)):
        mf.setParam(k, v)
    mf.setParam("passTimings", 1)
    obj = []
    for k in range(12):
        rgb, d, m = st.frame(k)
        if k == 11:
            mf.setParam("batchObjectPasses", 0)
        mf.processFrame(rgb, d, mask=m, classIDs=[0, 41, 42, 43], timestamp=k)
        obj.append((len(mf.getModels()), mf.passTimings()["objFuseClean"]))
    print("models / objFuseClean per frame:", [(n, round(v, 4)) for n, v in obj])
    assert obj[10][0] >= 3 and obj[10][1] > 0        # two object models or more: one launch per pass for all of them
    assert obj[11][0] >= 3 and obj[11][1] == 0
    mf.close()
