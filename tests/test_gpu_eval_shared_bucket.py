"""The shared-bucket rule of the cloud grid's record walk (nn_walk_records in csrc/mf_eval.hip): two cells of one point's walk may hash to
the same bucket, and a sum -- the normals' neighbour count, the FPFH pair count -- must meet every record once all the same, while the
nearest-neighbour minimum may meet it twice.  A cloud of 24 points has B = 64 buckets for the 27 cells of a walk, so a shared bucket is the
rule; the test restates the hash, the cell assignment and the walk's bounds in numpy and proves, before it calls the library, that its cloud
has one with a record within the radius in it.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_restatement as fr  # noqa: E402
import normals_restatement as nr  # noqa: E402
from test_gpu_eval import brute  # noqa: E402

pytestmark = pytest.mark.gpu

N, RADIUS = 24, np.float32(0.25)
SEEDS = range(32)


def _buckets(n):
    b = 64
    while b < 2 * n:
        b <<= 1
    return b


def nn_hash(x, y, z):
    """nn_hash of csrc/mf_eval.hip on Python ints (uint32 arithmetic)"""
    M = 0xFFFFFFFF
    h = ((x & M) * 0x8da6b343 ^ (y & M) * 0xd8163841 ^ (z & M) * 0xcb1ab31f) & M
    h ^= h >> 16
    h = h * 0x7feb352d & M
    h ^= h >> 15
    h = h * 0x846ca68b & M
    h ^= h >> 16
    return h


def _cells(p, radius):
    """nn_cell per axis: floor(x * (1 / radius)) in fp64"""
    return np.floor(p.astype(np.float64) * (1.0 / float(radius))).astype(np.int64)


def _walk(x, radius):
    """the cells nn_walk_cells visits for point x with the limit r2: nn_cell_range's bounds, less the cells beyond nn_box_gap"""
    h, r2 = float(radius), float(np.float32(radius) * np.float32(radius))
    inv_h, reach, pad = 1.0 / h, h * (1.0 + 2.0 ** -20), h * 2.0 ** -20
    x = x.astype(np.float64)
    lo, hi = np.floor((x - reach) * inv_h).astype(np.int64), np.floor((x + reach) * inv_h).astype(np.int64)

    def gap(v, c):
        a, b = c * h - pad, (c + 1) * h + pad
        d = a - v if v < a else (v - b if v > b else 0.0)
        return d * d
    return [(cx, cy, cz) for cz in range(lo[2], hi[2] + 1) for cy in range(lo[1], hi[1] + 1) for cx in range(lo[0], hi[0] + 1)
            if (gap(x[2], cz) + gap(x[1], cy) + gap(x[0], cx)) * (1.0 - 2.0 ** -18) <= r2]


def _shared_bucket_points(pts, radius):
    """the points i whose walk visits two distinct cells of one bucket, one of them holding a record within the radius of i"""
    mask = _buckets(len(pts)) - 1
    cell = [tuple(c) for c in _cells(pts, radius)]
    near = nr.neighbour_mask(pts, radius, np.arange(len(pts)))
    out = []
    for i in range(len(pts)):
        walk = _walk(pts[i], radius)
        assert len(walk) <= 27
        bucket = {}
        for c in walk:
            bucket.setdefault(nn_hash(*c) & mask, []).append(c)
        held = {cell[j] for j in np.flatnonzero(near[i])}
        if any(len(cs) > 1 and held.intersection(cs) for cs in bucket.values()):
            out.append(i)
    return out


def _cloud(seed):
    """24 points in a cube of edge RADIUS about a corner of the grid: eight cells hold them"""
    rng = np.random.default_rng(seed)
    corner = RADIUS * rng.integers(-8, 9, 3).astype(np.float32)
    return (corner + rng.uniform(-0.5, 0.5, (N, 3)).astype(np.float32) * RADIUS).astype(np.float32)


def _qualifying_cloud():
    for seed in SEEDS:
        pts = _cloud(seed)
        shared = _shared_bucket_points(pts, RADIUS)
        if shared:
            return pts, shared
    pytest.fail(f"no seed of {list(SEEDS)} gives a cloud with a shared bucket in a walk")


def test_sums_meet_a_record_once_where_two_cells_share_a_bucket(hip):
    from maskfusion_amd import eval as ev
    pts, shared = _qualifying_cloud()
    assert len(pts) == N and np.isfinite(pts).all() and _buckets(N) == 64
    assert (np.ptp(pts, 0) <= RADIUS).all() and len({tuple(c) for c in _cells(pts, RADIUS)}) > 1      # one cube, more than one cell
    assert shared
    near = nr.neighbour_mask(pts, RADIUS, np.arange(N))
    print("points with a shared bucket in their walk:", shared, "neighbours:", near.sum(1).tolist())
    # the normals' count: the neighbours within the radius, the point included
    _, _, cnt = ev.estimate_normals(pts, RADIUS)
    assert cnt.tolist() == near.sum(1).tolist()
    # the FPFH pair count k: the brute-force restatement's, and with normals in general position every neighbour but the point itself
    rng = np.random.default_rng(7)
    nrm = rng.normal(size=(N, 3)).astype(np.float32)
    _, spfh = ev.fpfh(pts, nrm, RADIUS)
    want = fr.fpfh(pts, nrm, RADIUS)["spfh"]
    assert spfh[:, 33].tolist() == want[:, 33].tolist() == (near.sum(1) - 1).tolist()
    assert (spfh[:, :33].reshape(N, 3, 11).sum(2) == spfh[:, 33:]).all()
    # the minimum: the cloud against itself, and against queries between its points
    for q in (pts, (pts + rng.uniform(-0.4, 0.4, (N, 3)).astype(np.float32) * RADIUS).astype(np.float32)):
        dist, idx = ev.nearest(pts, q, RADIUS)
        bd, bi = brute(pts, q, RADIUS)
        assert idx.tolist() == bi.tolist() and dist.tobytes() == bd.tobytes()
    assert ev.nearest(pts, pts, RADIUS)[1].tolist() == list(range(N))


@pytest.mark.parametrize("n", [1, 0])
def test_one_point_and_no_point(hip, n):
    from maskfusion_amd import eval as ev
    pts = _cloud(0)[:n]
    nrm = np.ones((n, 3), np.float32)
    normals, var, cnt = ev.estimate_normals(pts, RADIUS)
    assert normals.shape == (n, 3) and var.shape == (n,) and cnt.tolist() == [1] * n and np.isnan(normals).all() and np.isnan(var).all()
    desc, spfh = ev.fpfh(pts, nrm, RADIUS)
    assert desc.shape == (n, 33) and np.isnan(desc).all() and spfh.shape == (n, 34) and not spfh.any()
    q = _cloud(1)[:5]
    dist, idx = ev.nearest(pts, q, RADIUS)
    bd, bi = brute(pts, q, RADIUS)
    assert idx.tolist() == bi.tolist() and dist.tobytes() == bd.tobytes()
    dist, idx = ev.nearest(pts, pts, RADIUS)
    assert idx.tolist() == list(range(n)) and (dist == 0).all()
