"""The objects of the re-detection tests (tests/test_gpu_redetect.py) as downloadMap records: the asymmetric scene of tests/global_scene.py
scaled to 0.5 m as about 6 000 surfels, its image under global_scene.motion() scaled alike, a negative control -- the same scene without its
sphere and its box and with one wall 3 m long instead of 2 m, so that a seventh of it has no partner on the object -- and a noisy, partial
second sample."""
from __future__ import annotations

import numpy as np

import global_scene as gs

SCALE = 0.25                       # the scene is 2 m long
N = 6000


def records(points, normals, confidence=10.0, radius=0.004):
    """(n, 12) float32 in Model.downloadMap's layout: position + confidence | colour, unused, initTime, lastTime | normal + radius"""
    r = np.zeros((len(points), 12), np.float32)
    r[:, :3], r[:, 3] = points, confidence
    r[:, 4], r[:, 6], r[:, 7] = float(0x808080), 1.0, 1.0
    r[:, 8:11], r[:, 11] = normals, radius
    return r


def motion():
    """global_scene.motion() at the objects' scale: new -> old"""
    T = gs.motion().copy()
    T[:3, 3] *= SCALE
    return T


def object_records(n=N, seed=5):
    p, nm = gs.scene(n, seed)
    return records(p * np.float32(SCALE), nm)


def negative_records(n=N, seed=5):
    rng = np.random.default_rng(seed)
    rects = [((0, 0, 0), (2.0, 0, 0), (0, 1.4, 0), (0, 0, 1)), ((0, 0, 0), (0, 1.4, 0), (0, 0, 1.0), (1, 0, 0)),
             ((0, 0, 0), (3.0, 0, 0), (0, 0, 0.7), (0, 1, 0))]                     # the last wall: 3 m, not 2 m
    areas = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v, _ in rects])
    counts = np.round(n * areas / areas.sum()).astype(int)
    P, Nm = zip(*[gs._rect(rng, c, o, u, v, nm) for (o, u, v, nm), c in zip(rects, counts)])
    return records((np.concatenate(P) * SCALE).astype(np.float32), np.concatenate(Nm).astype(np.float32))


def moved_records(rec, T):
    """the records' exact image under T (positions and normals)"""
    out = rec.copy()
    out[:, :3] = gs.moved(rec[:, :3], T)
    out[:, 8:11] = (rec[:, 8:11].astype(np.float64) @ T[:3, :3].T).astype(np.float32)
    return out


def noisy_records(T, n=N, sigma=1e-3, seed=6):
    """another sample of the object with `sigma` of noise, the 70 % of its points with the smallest x + y, under T"""
    p, nm = gs.scene(n, seed + 1)
    rng = np.random.default_rng(seed + 2)
    p = (p * np.float32(SCALE) + rng.normal(scale=sigma, size=p.shape)).astype(np.float32)
    s = p[:, 0] + p[:, 1]
    keep = s <= np.quantile(s, 0.7)
    return moved_records(records(p[keep], nm[keep]), T)
