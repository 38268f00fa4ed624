"""Every launch form a frame size can select, against the CPU oracle (oracle/).

Many kernels take their launch form from the image size: threads per workgroup, pixel slots per thread, chunk length, partial tiles, empty
trailing workgroups.  The other oracle comparisons run at 640x480, 1280x960 and 320x240 only; here the sizes are chosen by the form they select:

  geometric Gauss-Newton kernel k_icp_iter<threads, slots> (mf_k_icp_launch_form tells which one a size gets; ICP_SIZES below):
      328x248  <256, 1>  the last chunk holds 192 of 256 pixels
      352x240  <256, 2>  the only form that skips idle slots by wavefront; 264 of 320 workgroups hold pixels (as 848x480 at level 1, 424x240 at level 0)
      480x256  <512, 2>  chunk 512: the second slot idles in every workgroup
      416x296  <512, 2>  chunk 576, 214 of 240 workgroups hold pixels (as 512x424 at level 0)
      520x480  <512, 3>  chunk 1088: the third slot is 64 pixels wide, 230 of 240 workgroups hold pixels
      776x480  <512, 3>  243 workgroups: more than one round
  preprocessing at 424x240 (width = 40 mod 64, 26.5 sprite tile columns, a 106x60 level 2), 328x248 (partial tiles in both directions) and 40x24
  (narrower than one bilateral tile, shorter than the 13-tap window plus halo), and five frames of the whole pipeline at 424x240 and 416x296;
  SO(3) pre-alignment at 106x60 (a partial last workgroup) and 520x256 (more pixels than 512 workgroups of 256 threads: the grid strides).

Tolerances are those of the counterparts in test_gpu_kernels.py / test_gpu_rgbd.py / test_gpu_multimodel.py / test_gpu_pipeline.py; none is new.
Runs on the CPU-executed build too (MF_EMU=1, tests/test_emu_launch_forms.py)."""
import ctypes as C

import numpy as np
import pytest

from gpu_util import EMU, dev, empty, host, model_maps, nan_equal_close, scene_frames

pytestmark = pytest.mark.gpu

# size -> (threads, pixel slots the chunk needs, workgroups past the image?)
ICP_SIZES = {
    (328, 248): (256, 1, False),
    (352, 240): (256, 2, True),
    (480, 256): (512, 1, False),
    (416, 296): (512, 2, True),
    (520, 480): (512, 3, True),
    (776, 480): (512, 3, False),
}
# what launch_icp_iteration can dispatch: k_icp_iter<256, 1>, <256, 2>, <512, 2> (one or two slots in use) and <512, 3>
ICP_FORMS = {(256, 1), (256, 2), (512, 1), (512, 2), (512, 3)}
PRE_SIZES = [(424, 240), (328, 248), (40, 24)]
ANGLE = float(np.sin(np.float32(20.0 * 3.14159254 / 180.0)))


def _form(hip, W, H):
    out = np.zeros(5, np.int32)
    assert hip.mf_k_icp_launch_form(W, H, out.ctypes.data) == 0
    return dict(zip(("threads", "slots", "blocks", "chunk", "live"), (int(v) for v in out)))


# ------------------------------------------------------------------------------------------------
# B1: which form each size selects
# ------------------------------------------------------------------------------------------------
def test_sizes_cover_every_icp_launch_form(hip):
    seen = set()
    for (W, H), (threads, slots, idle_tail) in ICP_SIZES.items():
        f = _form(hip, W, H)
        print(W, H, f)
        assert (f["threads"], f["slots"]) == (threads, slots), ((W, H), f)
        assert (f["live"] < f["blocks"]) == idle_tail, ((W, H), f)
        # the accessor's own consistency: the chunks cover the image, `live` of them start inside it, a thread has a slot for every pixel
        P = W * H
        assert f["chunk"] % 64 == 0 and f["blocks"] * f["chunk"] >= P
        assert (f["live"] - 1) * f["chunk"] < P <= f["live"] * f["chunk"]
        assert (f["slots"] - 1) * f["threads"] < f["chunk"] <= f["slots"] * f["threads"]
        seen.add((f["threads"], f["slots"]))
    assert seen == ICP_FORMS
    # the details the cases below rely on
    assert _form(hip, 328, 248)["chunk"] == 256 and 328 * 248 % 256 == 192
    assert (_form(hip, 352, 240)["chunk"], _form(hip, 352, 240)["live"], _form(hip, 352, 240)["blocks"]) == (320, 264, 320)
    assert (_form(hip, 416, 296)["chunk"], _form(hip, 416, 296)["live"], _form(hip, 416, 296)["blocks"]) == (576, 214, 240)
    assert _form(hip, 520, 480)["chunk"] == 1088
    assert _form(hip, 776, 480)["blocks"] == 243
    # the sizes the sensors deliver select forms of the list: 848x480 at level 1 and 424x240 / 352x288 at level 0 -> <256, 2>; 512x424 -> <512, 2>
    for (W, H), want in (((424, 240), (256, 2)), ((352, 288), (256, 2)), ((512, 424), (512, 2)), ((640, 480), (512, 3)), ((320, 240), (256, 1)),
                         ((160, 120), (256, 1))):
        f = _form(hip, W, H)
        assert (f["threads"], f["slots"]) == want, ((W, H), f)
    assert hip.mf_k_icp_launch_form(0, 240, np.zeros(5, np.int32).ctypes.data) != 0
    assert hip.mf_k_icp_launch_form(320, 240, None) != 0


# ------------------------------------------------------------------------------------------------
# B2: one ICP step per size
# ------------------------------------------------------------------------------------------------
_icp_inputs = {}


def _icp_case(oracle, W, H):
    """frame pair -> (intrinsics, vc, nc, vp, np), built once per size and never modified (the variants copy vc)"""
    if (W, H) not in _icp_inputs:
        st, fr = scene_frames(2, W=W, H=H, noise=True)
        k = [st.fx, st.fy, st.cx, st.cy]
        dF0, dF1 = oracle.bilateral(fr[0][1]), oracle.bilateral(fr[1][1])
        vc = oracle.create_vmap(dF1, *k, 3.0)
        nc = oracle.create_nmap(vc)
        vp = oracle.create_vmap(dF0, *k, 20.0)
        npv = oracle.create_nmap(vp)
        _icp_inputs[(W, H)] = (k, vc, nc, vp, npv)
    return _icp_inputs[(W, H)]


def _icp_compare(hip, oracle, W, H, k, vc, nc, vp, npv, what, min_inliers):
    """test_gpu_kernels.py::test_icp_step's poses, gates and assertions"""
    from maskfusion_amd import synth
    T = synth.make_pose(synth.rot_xyz(0.004, -0.003, 0.002), [0.003, -0.002, 0.001])
    Rcurr, tcurr = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
    Rpi, tprev = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    A, b, res = oracle.icp_step(Rcurr, tcurr, vc, nc, Rpi, tprev, *k, vp, npv)
    assert res[1] >= min_inliers, (what, "the case must leave inliers to sum", res[1])
    out = empty(32)
    args = [np.ascontiguousarray(x.reshape(-1)) for x in (Rcurr, tcurr, Rpi, tprev)]
    d_vc, d_nc, d_vp, d_np = dev(vc), dev(nc), dev(vp), dev(npv)
    rc = hip.mf_k_icp_step(args[0].ctypes.data, args[1].ctypes.data, d_vc.data_ptr(), d_nc.data_ptr(), args[2].ctypes.data, args[3].ctypes.data,
                           *k, d_vp.data_ptr(), d_np.data_ptr(), 0.10, ANGLE, W, H, out.data_ptr(), None)
    assert rc == 0
    g = host(out)
    gA, gb, s = np.zeros((6, 6)), np.zeros(6), 0
    for i in range(6):
        for j in range(i, 7):
            if j == 6:
                gb[i] = g[s]
            else:
                gA[i, j] = gA[j, i] = g[s]
            s += 1
    scale = np.abs(A).max()
    eA = np.abs(gA - A).max() / scale
    eb = np.abs(gb - b).max() / max(np.abs(b).max(), 1e-3 * scale)
    er = abs(g[27] - res[0]) / max(res[0], 1e-9)
    print(f"{W}x{H} {what}: inliers device/oracle {g[28]:.0f}/{res[1]:.0f}  max|dA|/scale {eA:.2e}  max|db|/scale {eb:.2e}  |d sum r^2|/sum {er:.2e}")
    assert g[28] == res[1], "inlier count must match exactly"
    assert eA <= 1e-4
    assert eb <= 1e-4
    assert er <= 2e-5


@pytest.mark.parametrize("size", list(ICP_SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_icp_step_per_form(hip, oracle, size):
    """The whole image, then two variants of the same inputs in which one part of the launch carries the whole sum (the current frame's vertex
    map is NaN elsewhere): the last live workgroups alone (the partial last chunk, next to the workgroups past the image), and -- for a form
    with more than one pixel slot -- the slots above the first alone (pixels at offset >= threads of their chunk)."""
    W, H = size
    k, vc, nc, vp, npv = _icp_case(oracle, W, H)
    f = _form(hip, W, H)
    _icp_compare(hip, oracle, W, H, k, vc, nc, vp, npv, "all pixels", 1000)
    idx = np.arange(W * H).reshape(H, W)
    # tail: the last live workgroups, as many as hold at least eight image rows (the last row has no normals; a few hundred pixels gave no inlier)
    n_tail = max(3, -(-8 * W // f["chunk"]))
    tail = idx >= (f["live"] - n_tail) * f["chunk"]
    masks = [("tail workgroups", tail)]
    if f["slots"] > 1:
        masks.append(("upper slots", (idx % f["chunk"]) >= f["threads"]))
    for what, keep in masks:
        v = vc.copy()
        v[:, ~keep] = np.nan
        _icp_compare(hip, oracle, W, H, k, v, nc, vp, npv, what, 32)


# ------------------------------------------------------------------------------------------------
# C1: SO(3) pre-alignment -- a partial last workgroup, and an image above kSo3MaxBlocks * 256 pixels
# ------------------------------------------------------------------------------------------------
def _so3_compare(hip, last2, next2, k2, what):
    """test_gpu_rgbd.py::test_so3_prealign's assertions"""
    from oracle import mfo_rgbd
    Rr, er, cr, itr = mfo_rgbd.so3_prealign(last2, next2, *k2)
    assert cr > 0 and itr >= 1, (what, cr, itr)
    R, stats = np.zeros(9, np.float64), np.zeros(3, np.float32)
    d_l, d_n = dev(last2), dev(next2)
    H2, W2 = last2.shape
    assert hip.mf_k_so3_prealign(d_l.data_ptr(), d_n.data_ptr(), W2, H2, *[C.c_float(v) for v in k2], R.ctypes.data, stats.ctypes.data, None) == 0
    print(f"so3 {W2}x{H2} {what}: iterations {int(stats[2])}/{itr} count {stats[1]:.0f}/{cr:.0f} error {stats[0]:.6g}/{er:.6g} "
          f"max|dR| {np.abs(R.reshape(3, 3) - Rr).max():.2e}")
    assert int(stats[2]) == itr
    assert stats[1] == cr
    assert abs(stats[0] - er) <= 1e-5 * max(er, 1e-6)
    assert np.abs(R.reshape(3, 3) - Rr).max() < 2e-6


def test_so3_prealign_partial_last_workgroup(hip, oracle):
    """106x60, level 2 of a 424x240 frame: 6 360 pixels are 24 workgroups and 216 of the 25th's 256 threads"""
    from oracle import mfo_rgbd
    st, fr = scene_frames(4, W=424, H=240)
    pyr = [mfo_rgbd.u8_pyramid(mfo_rgbd.image_to_intensity(f[0])) for f in fr]
    assert pyr[0][2].shape == (60, 106)
    k2 = (st.fx / 4, st.fy / 4, st.cx / 4, st.cy / 4)
    for a, b in ((0, 1), (1, 3)):
        _so3_compare(hip, pyr[a][2], pyr[b][2], k2, f"frames {a}->{b}")


def test_so3_prealign_above_one_pixel_per_thread(hip, oracle):
    """520x256 = 133 120 pixels, above the 131 072 that 512 workgroups of 256 threads hold one each: the workgroups stride, threads 0..2047 of the
    grid carry two pixels.  The pair is the 520x256 window around the principal point of two consecutive 640x480 frames' level-1 intensity images
    enlarged twice (each texel repeated 2x2): a real motion with the smooth gradients of a coarse level."""
    from oracle import mfo_rgbd
    st, fr = scene_frames(2)
    lvl1 = [mfo_rgbd.u8_pyramid(mfo_rgbd.image_to_intensity(f[0]))[1] for f in fr]
    W2, H2 = 520, 256
    x0, y0 = (640 - W2) // 2, (480 - H2) // 2
    pair = [np.ascontiguousarray(np.repeat(np.repeat(im, 2, axis=0), 2, axis=1)[y0:y0 + H2, x0:x0 + W2]) for im in lvl1]
    assert pair[0].shape == (H2, W2) and W2 * H2 > 512 * 256
    _so3_compare(hip, pair[0], pair[1], (st.fx, st.fy, st.cx - x0, st.cy - y0), "window of an enlarged level 1")


# ------------------------------------------------------------------------------------------------
# B3: preprocessing at sizes with partial tiles
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=PRE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def pre(request):
    W, H = request.param
    st, fr = scene_frames(1, W=W, H=H, noise=True)
    return st, fr[0]


def _with_edge_defects(depth):
    """holes and depths below the filter's 0.03 gate in the interior AND on the last columns / rows (the partial tiles of every tiling)"""
    H, W = depth.shape
    d = depth.copy()
    d[H // 3:H // 3 + max(2, H // 12), W // 4:W // 4 + max(3, W // 10)] = 0.0      # interior hole
    d[H // 2, :] = 0.02                                                            # a row below the gate
    d[H - 3:, W - 11:W - 4] = 0.0                                                  # hole on the last rows
    d[H // 5:H // 5 + 5, W - 2:] = 0.0                                             # hole on the last columns
    d[H - 1, :W // 3] = 0.02                                                       # last row, below the gate
    d[2 * H // 3:, W - 1] = 0.02                                                   # last column, below the gate
    return d


def test_bilateral_partial_tiles(hip, oracle, pre):
    st, (_, depth, _) = pre
    depth = _with_edge_defects(depth)
    ref = oracle.bilateral(depth)
    d, out = dev(depth), empty(depth.shape)
    assert hip.mf_k_bilateral(d.data_ptr(), out.data_ptr(), st.W, st.H, None) == 0
    got = host(out)
    err, bad = nan_equal_close(got, ref, 2e-5, 1e-6)
    print(f"{st.W}x{st.H} bilateral max abs err", err)
    assert bad == 0
    assert ((got == 0) == (ref == 0)).all()
    assert (ref[:, -1] != 0).any() and (ref[-1] != 0).any() and (ref[-1] == 0).any() and (ref[:, -1] == 0).any()


def test_pyrdown_partial_tiles(hip, oracle, pre):
    st, (_, depth, _) = pre
    src = oracle.bilateral(_with_edge_defects(depth))
    src[st.H // 4:st.H // 4 + 3, st.W // 3:st.W // 3 + 5] = np.nan
    src[st.H - 2:, st.W // 2:st.W // 2 + 4] = np.nan
    for _ in range(2):
        ref = oracle.pyrdown_f(src)
        out, d = empty(ref.shape), dev(src)
        assert hip.mf_k_pyrdown_f(d.data_ptr(), out.data_ptr(), src.shape[1], src.shape[0], None) == 0
        err, bad = nan_equal_close(host(out), ref, 2e-6, 1e-7)
        print(f"pyrdown {src.shape[1]}x{src.shape[0]} max abs err", err)
        assert bad == 0
        src = ref


def test_vmap_nmap_partial_tiles(hip, oracle, pre):
    st, (_, depth, _) = pre
    depth = oracle.bilateral(_with_edge_defects(depth))
    for lvl in range(3):
        W, H = st.W >> lvl, st.H >> lvl
        k = [st.fx / (1 << lvl), st.fy / (1 << lvl), st.cx / (1 << lvl), st.cy / (1 << lvl)]
        v_ref = oracle.create_vmap(depth, *k, 3.0)
        n_ref = oracle.create_nmap(v_ref)
        v, n, d = empty((3, H, W)), empty((3, H, W)), dev(depth)
        assert hip.mf_k_vmap_nmap(d.data_ptr(), v.data_ptr(), n.data_ptr(), W, H, *k, 3.0, None) == 0
        ev, bv = nan_equal_close(host(v), v_ref, 2e-6, 1e-7)
        en, bn = nan_equal_close(host(n), n_ref, 5e-5, 1e-5)
        print(f"{W}x{H} vmap err", ev, "nmap err", en)
        assert bv == 0 and bn == 0
        depth = oracle.pyrdown_f(depth)


def test_model_pyramid_partial_tiles(hip, oracle, pre):
    from maskfusion_amd import synth
    st, (_, depth, _) = pre
    v4, n4 = model_maps(oracle, st, _with_edge_defects(depth))
    T = synth.make_pose(synth.rot_xyz(0.02, -0.03, 0.01), [0.05, -0.02, 0.03])
    R, t = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
    vs, ns = [None] * 3, [None] * 3
    vs[0], ns[0] = oracle.copy_maps(v4, n4)
    for i in (1, 2):
        vs[i] = oracle.resize_map(vs[i - 1], False)
        ns[i] = oracle.resize_map(ns[i - 1], True)
    ref = [oracle.transform_maps(vs[i], ns[i], R, t) for i in range(3)]
    tot = sum((st.W >> i) * (st.H >> i) * 3 for i in range(3))
    dv, dn = empty(tot), empty(tot)
    Rc = np.ascontiguousarray(R.reshape(9))
    d_v4, d_n4 = dev(v4), dev(n4)
    assert hip.mf_k_model_pyramid(d_v4.data_ptr(), d_n4.data_ptr(), Rc.ctypes.data, t.ctypes.data, dv.data_ptr(), dn.data_ptr(), st.W, st.H, None) == 0
    gv, gn = host(dv), host(dn)
    off = 0
    for i in range(3):
        sz = (st.W >> i) * (st.H >> i) * 3
        ev, bv = nan_equal_close(gv[off:off + sz].reshape(ref[i][0].shape), ref[i][0], 2e-6, 2e-6)
        en, bn = nan_equal_close(gn[off:off + sz].reshape(ref[i][1].shape), ref[i][1], 2e-5, 2e-6)
        print(f"{st.W}x{st.H} level", i, "v err", ev, "n err", en)
        assert bv == 0 and bn == 0
        off += sz


def test_intensity_pyramid_derivatives_partial_tiles(hip, oracle, pre):
    """exact, as test_gpu_rgbd.py::test_intensity_pyramid_derivatives"""
    import torch
    from oracle import mfo_rgbd
    st, _ = pre
    W, H = st.W, st.H
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[H // 6:H // 4, W // 3:W // 2] = 0            # zero texels are skipped by the pyramid: in the interior ...
    img[H - 3:, W - 9:] = 0                          # ... and in the last tile's corner
    img[0, :, :] = np.tile(np.arange(256, dtype=np.uint8), 4)[:W, None]     # grey ramp
    for ch, src in ((3, img), (4, np.concatenate([img, np.full((H, W, 1), 255, np.uint8)], axis=2))):
        d_img, d_out = dev(src), empty((H, W), torch.uint8)
        assert hip.mf_k_intensity(d_img.data_ptr(), ch, d_out.data_ptr(), W * H, None) == 0
        gray = mfo_rgbd.image_to_intensity(src)
        assert np.array_equal(host(d_out), gray)
    d_g = dev(gray)
    d_p1, d_p2 = empty((H // 2, W // 2), torch.uint8), empty((H // 4, W // 4), torch.uint8)
    assert hip.mf_k_pyrdown_u8(d_g.data_ptr(), d_p1.data_ptr(), W, H, None) == 0
    assert hip.mf_k_pyrdown_u8(d_p1.data_ptr(), d_p2.data_ptr(), W // 2, H // 2, None) == 0
    r1 = oracle.pyrdown_u8(gray)
    r2 = oracle.pyrdown_u8(r1)
    assert np.array_equal(host(d_p1), r1) and np.array_equal(host(d_p2), r2)
    for g in (gray, r1, r2):
        h, w = g.shape
        d_s, d_dx, d_dy = dev(g), empty((h, w), torch.int16), empty((h, w), torch.int16)
        assert hip.mf_k_derivative_images(d_s.data_ptr(), d_dx.data_ptr(), d_dy.data_ptr(), w, h, None) == 0
        rdx, rdy = mfo_rgbd.derivative_images(g)
        assert np.array_equal(host(d_dx), rdx) and np.array_equal(host(d_dy), rdy), (w, h)


def test_geometric_edges_partial_tiles(hip, oracle, pre):
    """as test_gpu_multimodel.py::test_geometric_edges_kernel"""
    import torch
    from oracle import mfo_mm
    st, (_, depth, _) = pre
    dF = oracle.bilateral(_with_edge_defects(depth))
    v = oracle.create_vmap(dF, st.fx, st.fy, st.cx, st.cy, 3.0)
    n = oracle.create_nmap(v)
    for (wD, wC, thr, rad, it) in ((150.0, 2.8, 0.3, 1, 0), (1.0, 1.0, 0.1, 1, 3), (150.0, 2.8, 0.3, 2, 1)):
        e_ref = mfo_mm.geometric_edge_map(v, n, wD, wC)
        _, inv_ref = mfo_mm.edge_binary(e_ref, thr, rad, it)
        d_v, d_n = dev(v), dev(n)
        d_e, d_b, d_t = empty((st.H, st.W)), empty((st.H, st.W), torch.uint8), empty((st.H, st.W), torch.uint8)
        assert hip.mf_k_geometric_edges(d_v.data_ptr(), d_n.data_ptr(), d_e.data_ptr(), d_b.data_ptr(), d_t.data_ptr(), st.W, st.H, wD, wC, thr, rad,
                                        it, None) == 0
        e, b = host(d_e), host(d_b)
        err, bad = nan_equal_close(e, e_ref, 1e-4, 1e-5)
        flips = (b != inv_ref)
        near = np.abs(e_ref - thr) < 1e-4
        print(f"{st.W}x{st.H} edge err", err, "binary flips", int(flips.sum()))
        assert bad == 0
        if it == 0:
            assert not (flips & ~near).any()
        else:
            assert flips.mean() < 1e-4


# ------------------------------------------------------------------------------------------------
# B4: the whole pipeline
# ------------------------------------------------------------------------------------------------
PIPELINE_FRAMES = 5


def _pipeline(oracle, W, H, icp_weight, so3, n_frames):
    """test_gpu_pipeline.py::_run at another size, plus the filtered depth of frames 0 and 1 and the frame's own maps after frame 1"""
    from maskfusion_amd import MaskFusion
    st, frames = scene_frames(n_frames, W=W, H=H, noise=True)
    cap = 1 << 19
    o = oracle.Oracle(st.W, st.H, st.fx, st.fy, st.cx, st.cy, icpWeight=icp_weight, capacity=cap, so3=int(so3))
    m = MaskFusion(st.W, st.H, st.fx, st.fy, st.cx, st.cy, icpThresh=icp_weight, so3=bool(so3), numGSurfels=cap, enableMultipleModels=False)
    rec = dict(op=[], gp=[], oc=[], gc=[], ofill=[], gfill=[], o_depthF=[], g_depthF=[], st=st)
    for k, (rgb, depth, _) in enumerate(frames):
        o.process_frame(rgb, depth)
        m.processFrame(rgb, depth, timestamp=k)
        rec["op"].append(o.pose); rec["gp"].append(m.getCurrPose())
        rec["oc"].append(o.count); rec["gc"].append(m.getBackgroundModel().lastCount())
        rec["ofill"].append(o.dbg("fillin")); rec["gfill"].append(int(m.getLastFillIn()))
        if k <= 1:
            rec["o_depthF"].append(o.dbg("depthF")); rec["g_depthF"].append(m.debugRead("depthF"))
        if k == 1:   # (the frame that initialises the map is never tracked against: the first vertex / normal maps are frame 1's)
            rec["g_vmap"] = [m.debugRead(f"vmap{i}") for i in range(3)]
            rec["g_nmap"] = [m.debugRead(f"nmap{i}") for i in range(3)]
    o.close(); m.close()
    return rec


def _check_pipeline(oracle, rec, what):
    gp, op = np.array(rec["gp"]), np.array(rec["op"])
    d = np.linalg.norm(gp[:, :3, 3] - op[:, :3, 3], axis=1)
    dR = np.abs(gp[:, :3, :3] - op[:, :3, :3]).max(axis=(1, 2))
    gc, oc = np.array(rec["gc"], float), np.array(rec["oc"], float)
    print(f"{what}: per-frame |dt| (um)", np.round(d * 1e6, 2), "max |dR|", dR.max(), "counts device", rec["gc"], "oracle", rec["oc"])
    assert d[:5].max() < 1e-4 and dR[:5].max() < 1e-4      # frame 0 and the first four tracked frames
    assert rec["gfill"] == rec["ofill"]
    assert (np.abs(gc - oc) / oc).max() < 5e-3
    # The filter (frame 0: its own launch; frame 1: beside the binning of frame 0's prediction) against the oracle's at the filter's tolerance.  Then
    # frame 1's pyramid launch against the oracle's pyrDownGaussF / createVMap / createNMap at the kernel tests' tolerances, unchanged at every
    # level -- applied to the DEVICE's filtered depth (and, for a normal map, to the device's vertex map of its level), as those tests apply them
    # to the kernel's own input: the filter's own tolerance (2e-5) is ten times the vertex map's, and createNMap differences neighbouring vertices,
    # which amplifies a last-bit depth difference a thousandfold (test_gpu_pipeline.py::test_first_frame_init), so the oracle's chain from ITS
    # filtered depth cannot be held to them.  The error against that chain is printed (MI355X and the CPU-executed build alike, 424x240: vertex
    # maps 1.2e-6 / 9.5e-7 / 9.5e-7 at levels 0 / 1 / 2, normal maps 2.2e-4 / 7.1e-5 / 3.6e-5, NaN patterns equal).
    st = rec["st"]
    for g_d, o_d in zip(rec["g_depthF"], rec["o_depthF"]):
        err, bad = nan_equal_close(g_d, o_d, 2e-5, 1e-6)
        assert bad == 0
        assert ((g_d == 0) == (o_d == 0)).all()
    depth, o_depth = rec["g_depthF"][1], rec["o_depthF"][1]
    for lvl in range(3):
        k = [st.fx / (1 << lvl), st.fy / (1 << lvl), st.cx / (1 << lvl), st.cy / (1 << lvl)]
        v_ref = oracle.create_vmap(depth, *k, 3.0)
        ev, bv = nan_equal_close(rec["g_vmap"][lvl], v_ref, 2e-6, 1e-7)
        n_ref = oracle.create_nmap(rec["g_vmap"][lvl])
        en, bn = nan_equal_close(rec["g_nmap"][lvl], n_ref, 5e-5, 1e-5)
        v_own = oracle.create_vmap(o_depth, *k, 3.0)
        n_own = oracle.create_nmap(v_own)
        both_v, both_n = ~np.isnan(v_own) & ~np.isnan(rec["g_vmap"][lvl]), ~np.isnan(n_own) & ~np.isnan(rec["g_nmap"][lvl])
        print(f"{what}: frame 1 level {lvl} vmap err {ev:.2e} nmap err {en:.2e}; against the oracle's chain from its own filtered depth: "
              f"vmap {np.abs(rec['g_vmap'][lvl] - v_own)[both_v].max():.2e} nmap {np.abs(rec['g_nmap'][lvl] - n_own)[both_n].max():.2e}, "
              f"NaN pattern differs at {int((np.isnan(v_own) != np.isnan(rec['g_vmap'][lvl])).sum())} / "
              f"{int((np.isnan(n_own) != np.isnan(rec['g_nmap'][lvl])).sum())} entries")
        assert bv == 0 and bn == 0
        depth, o_depth = oracle.pyrdown_f(depth), oracle.pyrdown_f(o_depth)


@pytest.mark.parametrize("W,H,icp_weight,so3", [(424, 240, 100.0, False), (424, 240, 10.0, True), (416, 296, 100.0, False)],
                         ids=["424x240-icp", "424x240-rgbd-so3", "416x296-icp"])
def test_pipeline_per_form(hip, oracle, W, H, icp_weight, so3):
    """424x240: k_icp_iter<256, 2> at level 0 (and, with icpThresh 10 + SO(3), k_rgbd_iter / k_rgb_step on a grid with workgroups past the image
    and the pre-alignment's partial last workgroup); 416x296: <512, 2> with empty trailing workgroups at level 0"""
    import os
    # (the CPU-executed leg, and only it, may ask for fewer frames: tests/test_emu_launch_forms.py runs three)
    n = int(os.environ.get("MF_LAUNCH_FORM_FRAMES", PIPELINE_FRAMES)) if EMU else PIPELINE_FRAMES
    _check_pipeline(oracle, _pipeline(oracle, W, H, icp_weight, so3, n), f"{W}x{H} icpThresh {icp_weight:g} so3 {int(so3)}")
