"""Inputs of the cloud-visibility tests (tests/test_gpu_visibility.py): a random cloud that exercises every branch of the rule, the literal
decision edges, and a crafted scene whose observed part is known.  Built once per process; nobody writes into them."""
import functools

import numpy as np

from maskfusion_amd import synth
from maskfusion_amd import eval as ev

F32 = np.float32


def backproject(depth, T_wc, fx, fy, cx, cy, z=None):
    """the pixels of one depth image as world points, in fp64: (H * W, 3) in row-major pixel order (z: another depth along the same rays)"""
    H, W = depth.shape
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.asarray(depth if z is None else z, np.float64)
    cam = np.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], -1).reshape(-1, 3)
    return cam @ T_wc[:3, :3].T + T_wc[:3, 3]


# ---------------------------------------------------------------- the random cloud ----------------------------------------------------------------
RANDOM_N = 1061                                   # neither a multiple of 64 nor of 256
RANDOM_K = dict(fx=33.0, fy=33.0, cx=19.5, cy=14.5)
RANDOM_RULE = dict(near_z=0.02, far_z=6.0, tol_abs=0.02, tol_rel=0.01)
SHEET_FRAME = 2                                   # the frame whose depth is a sheet at 0.05 m


@functools.lru_cache(None)
def random_cloud():
    """(points (1061, 12) float32 with x y z first, depth (7, 30, 40), cam_from_cloud (7, 12)); the tests of the rule use the first five frames"""
    rng = np.random.default_rng(1061)
    st = synth.Stream(W=40, H=30, **RANDOM_K)
    ids = [0, 20, 40, 60, 80, 100, 120]
    depth = np.stack([st.frame(k)[1] for k in ids])
    poses = np.stack([st.gt_pose(k) for k in ids])
    n_seen = RANDOM_N // 3
    frame = rng.integers(0, 5, n_seen)
    pix = rng.integers(0, 40 * 30, n_seen)
    z = depth.reshape(7, -1)[frame, pix].astype(np.float64) + rng.uniform(-0.05, 0.05, n_seen)      # jittered along the ray
    near = rng.permutation(n_seen)[:n_seen // 10]
    z[near] = rng.uniform(0.1, 0.3, len(near))                                                       # a tenth: close to the camera, on their frame's ray
    seen = np.empty((n_seen, 3))
    for k in range(n_seen):
        img = np.zeros((30, 40))
        seen[k] = backproject(depth[frame[k]], poses[frame[k]], z=img + z[k], **RANDOM_K)[pix[k]]
    n_box = RANDOM_N // 3
    box = rng.uniform([-2.6, -1.6, -1.1], [2.6, 1.3, 2.9], (n_box, 3))
    n_rest = RANDOM_N - n_seen - n_box
    rest = np.where(rng.integers(0, 2, (n_rest, 1)) == 0, rng.uniform([-2, -1, -3], [2, 1, -0.5], (n_rest, 3)),      # behind the camera
                    rng.uniform(-1, 1, (n_rest, 3)) * 40 + 100)                                                     # far outside
    points = rng.uniform(-9, 9, (RANDOM_N, 12)).astype(F32)
    points[:, :3] = np.concatenate([seen, box, rest]).astype(F32)
    depth = depth.copy()
    depth[SHEET_FRAME] = F32(0.05)
    for f, (r0, c0, val) in enumerate([(3, 4, 0.0), (10, 20, -1.0), (0, 0, np.nan), (20, 30, np.inf), (12, 8, 0.0), (5, 5, np.nan), (25, 2, -1.0)]):
        depth[f, r0:r0 + 6, c0:c0 + 8] = val
    depth[0, 15:19, 10:14] = np.nan
    depth[1, 2:6, 30:36] = np.inf
    return points, depth, ev.cam_from_cloud(poses)


# ---------------------------------------------------------------- decision edges ----------------------------------------------------------------
EDGE_K = dict(fx=32.0, fy=32.0, cx=15.5, cy=11.5)
EDGE_W, EDGE_H = 32, 24
EDGE_RULE = dict(near_z=0.5, far_z=4.0, tol_abs=0.25, tol_rel=0.0)
EDGE_RULE_REL = dict(near_z=0.5, far_z=4.0, tol_abs=0.0, tol_rel=0.125)      # 0.125 * 2.0 = 0.25 exactly
OUT, THROUGH, ON, OCC = "out", "through", "on", "occluded"


def _up(x):
    return np.nextafter(F32(x), F32(np.inf))


def _down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def edge_cases():
    """[(x, y, z, expected class)] against a depth of 2.0 everywhere under the identity pose.  At z = 1: u + 0.5 = 32 x + 16 and
    v + 0.5 = 32 y + 12, every operation exact at the values below except where a comment says how it rounds.
    Left and top border: x = -0.5 gives u + 0.5 = 0, column 0.  One float below, 32 x + 15.5 = -0.5 - 2^-19 is exact (spacing 2^-24 there)
    and u + 0.5 = -2^-19: column -1.  One float above: +2^-20, column 0.
    Right and bottom border: x = 0.5 gives u + 0.5 = 32: column 32, outside.  One float below, 32 x = 16 - 2^-20 and 32 x + 15.5 =
    31.5 - 2^-20 lies half way between two floats (spacing 2^-19 there) and rounds to the even one, 31.5: u + 0.5 = 32 again, OUTSIDE -- the
    border is decided in fp32, not in the reals.  Two floats below: 31.5 - 2^-19, column 31.  The rows behave the same at y = -+0.375
    (32 y + 11.5 = 23.5 - 2^-20 is the same tie, 23.5 being even)."""
    nan, inf = F32(np.nan), F32(np.inf)
    c = []
    for k in range(2):                     # k = 0: x decides the column; k = 1: y decides the row
        h = F32(0.5) if k == 0 else F32(0.375)
        for t, want in [(-h, THROUGH), (_down(-h), OUT), (_up(-h), THROUGH), (h, OUT), (_down(h), OUT), (_down(_down(h)), THROUGH), (_up(h), OUT)]:
            c.append((t, 0.0, 1.0, want) if k == 0 else (0.0, t, 1.0, want))
    c += [(0.0, 0.0, 0.5, OUT), (0.0, 0.0, _up(0.5), THROUGH)]                     # zc == near is out, one float above is in
    c += [(0.0, 0.0, 4.0, OCC), (0.0, 0.0, _up(4.0), OUT)]                         # zc == far is in, one float above is out
    c += [(0.0, 0.0, 2.25, ON), (0.0, 0.0, 1.75, ON), (0.0, 0.0, _up(2.25), OCC), (0.0, 0.0, _down(1.75), THROUGH), (0.0, 0.0, 2.0, ON)]
    c += [(0.0, 0.0, 0.0, OUT), (0.0, 0.0, -1.0, OUT), (0.25, 0.25, -2.0, OUT)]
    for bad in (nan, inf, -inf):
        c += [(bad, 0.0, 1.0, OUT), (0.0, bad, 1.0, OUT), (0.0, 0.0, bad, OUT)]
    return c


EDGE_ROW = {OUT: (0, 0, 0, 0), ON: (1, 1, 0, 0), THROUGH: (1, 0, 1, 0), OCC: (1, 0, 0, 1)}


def edge_inputs():
    cases = edge_cases()
    points = np.array([c[:3] for c in cases], F32)
    depth = np.full((1, EDGE_H, EDGE_W), 2.0, F32)
    cam = ev.cam_from_cloud(np.eye(4))
    want = np.array([EDGE_ROW[c[3]] for c in cases], np.uint32)
    return points, depth, cam, want


# ---------------------------------------------------------------- the crafted scene ----------------------------------------------------------------
CRAFT_K = dict(fx=66.0, fy=66.0, cx=39.5, cy=29.5)
CRAFT_W, CRAFT_H = 80, 60
CRAFT_FRAMES = (0, 30, 60, 90)
CRAFT_SEEN = 19200
CRAFT_RULE = dict(near_z=0.01, far_z=10.0, tol_abs=0.002, tol_rel=0.0)


def crafted_from(depth, poses):
    """the reference cloud of the crafted scene for these four depth images: their valid pixels back-projected into the world, then 500 points
    behind the back wall (at z = 2.8), then 500 behind every camera"""
    rng = np.random.RandomState(0)
    seen = np.concatenate([backproject(d, T, **CRAFT_K)[(d > 0).reshape(-1)] for d, T in zip(depth, poses)])
    wall = np.stack([rng.uniform(-2, 2, 500), rng.uniform(-1, 1, 500), rng.uniform(3.0, 3.5, 500)], 1)
    behind = np.stack([rng.uniform(-2, 2, 500), rng.uniform(-1, 1, 500), rng.uniform(-0.9, -0.4, 500)], 1)
    return np.concatenate([seen, wall, behind]).astype(F32)


@functools.lru_cache(None)
def crafted():
    """(stream frames [(rgb, depth)], poses (4, 4, 4), reference (20200, 3) float32)"""
    st = synth.Stream(W=CRAFT_W, H=CRAFT_H, **CRAFT_K)
    frames = [st.frame(k)[:2] for k in CRAFT_FRAMES]
    poses = np.stack([st.gt_pose(k) for k in CRAFT_FRAMES])
    ref = crafted_from([f[1] for f in frames], poses)
    return frames, poses, ref
