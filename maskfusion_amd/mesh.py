"""Triangle meshes of surfel clouds: naive surface nets over a moving-least-squares signed distance to the surfels' tangent planes, on the
GPU (mf_cloud_mesh_build_dev / mf_cloud_mesh_emit_dev, kernels: csrc/mf_mesh.hip; the definition: include/maskfusion_amd.h; DESIGN.md "Surfel
meshing").

    python -m maskfusion_amd.mesh --cloud out/cloud-0.ply --voxel 0.01 -o out/mesh-0.ply

mesh_cloud() meshes oriented points, write_mesh_ply() writes the result as a binary PLY whose vertex element has mf_save_ply's property
names (so maskfusion_amd.eval.read_ply and every mesh viewer read it) followed by a `face` element.  MaskFusion.saveMesh (api.py) and the
command line's -emesh write one mesh-<id>.ply per model.  read_triangle_mesh() reads a mesh back from .ply or .obj (read_obj) for
maskfusion_amd.eval --ref-mesh; --fidelity adds the exact distances from the input points to the mesh just written (eval.TriMesh).

    python -m maskfusion_amd.mesh --mesh scene.obj --views seq/ --poses seq/groundtruth.txt

--views renders the mesh -- the one just written, or with --mesh an existing one -- from every frame's pose (eval.TriMesh.render: GPU ray
casting, mf_trimesh_render_dev; DESIGN.md "Mesh rendering") and scores depth and colour against the sensor's frames (eval.ViewScorer);
shade() turns a render's triangle indices and weights into colours on the host.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import sys

import numpy as np


class Mesh:
    """The library's handle of a built mesh (mf_mesh): the counts, emit() into device tensors, close()."""

    def __init__(self, records, normal_offset: int, color_offset: int, origin, voxel: float, dims, support: float, min_neighbours: int = 3,
                 stage_ms: bool = False):
        """records: (n, stride) float32 device tensor (or numpy array), x y z first; see mf_cloud_mesh_build_dev"""
        from .eval import _device_points, _stream_of
        from .lib import MF_MESH_STAGES, MFError, load
        self._L = load()
        self._h = C.c_void_p()
        rec = _device_points(records, 6, "records must be (n, >= 6) float32: x y z, a normal and optionally a colour")
        self.device = rec.device
        self._stream = _stream_of(rec.device)
        n = int(rec.shape[0])
        origin = np.ascontiguousarray(origin, np.float32).reshape(3)
        dims = np.ascontiguousarray(dims, np.int32).reshape(3)
        nv, nq = C.c_uint32(0), C.c_uint32(0)
        ms = np.zeros(MF_MESH_STAGES, np.float32)
        rc = self._L.mf_cloud_mesh_build_dev(rec.data_ptr() if n else None, int(rec.shape[1]), int(normal_offset), int(color_offset), n,
                                             origin.ctypes.data, float(voxel), dims.ctypes.data, float(support), int(min_neighbours),
                                             C.byref(self._h), C.byref(nv), C.byref(nq), ms.ctypes.data if stage_ms else None, self._stream)
        if rc != 0:
            raise MFError(f"mf_cloud_mesh_build_dev failed with code {rc}: {self._L.mf_last_error(None).decode()}")
        self.n_vertices, self.n_quads, self.has_color = int(nv.value), int(nq.value), color_offset >= 0
        self.stage_ms = ms if stage_ms else None

    def emit(self, normals: bool = True, colors: bool = True, cells: bool = False):
        """device tensors: vertices (nv, 3), normals (nv, 3) or None, colours (nv, 3) or None, cells (nv, 3) int32 or None, quads (nq, 4) int32"""
        import torch
        from .lib import MFError
        nv, nq, d = self.n_vertices, self.n_quads, self.device
        v = torch.empty((nv, 3), dtype=torch.float32, device=d)
        nr = torch.empty((nv, 3), dtype=torch.float32, device=d) if normals else None
        co = torch.empty((nv, 3), dtype=torch.float32, device=d) if colors and self.has_color else None
        ce = torch.empty((nv, 3), dtype=torch.int32, device=d) if cells else None
        q = torch.empty((nq, 4), dtype=torch.int32, device=d)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        rc = self._L.mf_cloud_mesh_emit_dev(self._h, ptr(v), ptr(nr), ptr(co), ptr(ce), ptr(q), self._stream)
        if rc != 0:
            raise MFError(f"mf_cloud_mesh_emit_dev failed with code {rc}: {self._L.mf_last_error(None).decode()}")
        return v, nr, co, ce, q

    def close(self):
        if self._h:
            self._L.mf_cloud_mesh_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lattice_for(points, normals, voxel: float, support: float):
    """(origin float32[3], dims int32[3]) of the lattice that covers the eligible points' bounding box grown by `support`; None when no point
    is eligible.  points, normals: torch tensors (n, 3) on any device."""
    import torch
    ok = torch.isfinite(points).all(1) & torch.isfinite(normals).all(1) & (normals != 0).any(1)
    if not bool(ok.any()):
        return None
    p = points[ok].double()
    lo = (p.min(0).values - support).cpu().numpy()
    hi = (p.max(0).values + support).cpu().numpy()
    origin = lo.astype(np.float32)
    dims = np.ceil((hi - origin.astype(np.float64)) / voxel).astype(np.int64) + 2
    return origin, np.maximum(dims, 2).astype(np.int32)


def quads_to_triangles(quads: np.ndarray) -> np.ndarray:
    """each quad (0, 1, 2, 3) as the triangles (0, 1, 2), (0, 2, 3)"""
    q = np.asarray(quads, np.int32).reshape(-1, 4)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3)


def mesh_cloud(points, normals, colors=None, voxel: float = 0.01, support: float | None = None, min_neighbours: int = 3, origin=None, dims=None,
               return_quads: bool = False):
    """Meshes oriented points.  points, normals (n, 3), colors (n, 3) in any linear scale or None; numpy arrays or torch tensors.  support
    defaults to 2.5 voxel; origin / dims default to lattice_for().  Returns numpy (vertices (nv, 3) float32, normals (nv, 3) float32,
    colours (nv, 3) float32 or None, triangles (nt, 3) int32) -- with return_quads=True the quads (nq, 4) instead of the triangles and
    the vertices' lattice cells (nv, 3) int32 as a fifth value."""
    import torch
    from .lib import torch_device
    support = 2.5 * voxel if support is None else support
    dev = torch_device()
    as_t = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32)))).to(dev).float().reshape(-1, 3)  # noqa: E731
    cols = [as_t(points), as_t(normals)] + ([as_t(colors)] if colors is not None else [])
    if len({int(c.shape[0]) for c in cols}) != 1:
        raise ValueError("points, normals and colours must have the same number of rows")
    if origin is None or dims is None:
        lat = lattice_for(cols[0], cols[1], float(voxel), float(support)) if math.isfinite(voxel) and voxel > 0 and math.isfinite(support) else None
        origin, dims = lat if lat is not None else (np.zeros(3, np.float32), np.full(3, 2, np.int32))
    rec = torch.cat(cols, 1).contiguous()
    with Mesh(rec, 3, 6 if colors is not None else -1, origin, voxel, dims, support, min_neighbours) as m:
        v, nr, co, ce, q = m.emit(cells=return_quads)
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    if return_quads:
        return host(v), host(nr), host(co), host(q), host(ce)
    return host(v), host(nr), host(co), quads_to_triangles(host(q))


def write_mesh_ply(path: str, vertices, normals=None, colors=None, triangles=None):
    """Binary little-endian PLY: `vertex` first -- x y z, then red green blue (uchar; colours are clipped to 0..255 and rounded) when there
    are colours, then nx ny nz when there are normals: mf_save_ply's names and order -- then `face` with `vertex_indices` (uchar count,
    int indices)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    fields, cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")], [v[:, 0], v[:, 1], v[:, 2]]
    head = ["property float x", "property float y", "property float z"]
    if colors is not None:
        c = np.clip(np.rint(np.nan_to_num(np.asarray(colors, np.float64).reshape(-1, 3))), 0, 255).astype(np.uint8)
        for k, nm in enumerate(("red", "green", "blue")):
            fields.append((nm, "u1")); cols.append(c[:, k]); head.append(f"property uchar {nm}")
    if normals is not None:
        nr = np.asarray(normals, np.float32).reshape(-1, 3)
        for k, nm in enumerate(("nx", "ny", "nz")):
            fields.append((nm, "<f4")); cols.append(nr[:, k]); head.append(f"property float {nm}")
    rec = np.empty(len(v), np.dtype(fields))
    for (nm, _), col in zip(fields, cols):
        rec[nm] = col
    t = np.zeros((0, 3), np.int32) if triangles is None else np.asarray(triangles, np.int32).reshape(-1, 3)
    faces = np.empty(len(t), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    faces["n"] = 3
    faces["i"] = t
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%s\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n"
                 % (len(v), "\n".join(head), len(t))).encode("ascii"))
        f.write(rec.tobytes())
        f.write(faces.tobytes())


def read_mesh_ply(path: str):
    """What write_mesh_ply wrote: a dict with vertices, normals / colors (None when absent) and triangles"""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    at = raw.index(b"\n", end) + 1
    lines = raw[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary little-endian files are read")
    types = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    counts, props, cur = {}, {"vertex": [], "face": []}, None
    for line in lines:
        w = line.split()
        if w[:1] == ["element"]:
            cur = w[1]
            counts[cur] = int(w[2])
            props.setdefault(cur, [])
        elif w[:1] == ["property"] and cur is not None:
            props[cur].append(w[1:])
    if list(counts)[:2] != ["vertex", "face"] or props["face"] != [["list", "uchar", "int", "vertex_indices"]]:
        raise ValueError(f"{path}: expected a vertex element, then faces with `property list uchar int vertex_indices`")
    vt = np.dtype([(p[1], types[p[0]]) for p in props["vertex"]])
    v = np.frombuffer(raw, vt, counts["vertex"], at)
    ft = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    fa = np.frombuffer(raw, ft, counts["face"], at + vt.itemsize * counts["vertex"])
    if counts["face"] and (fa["n"] != 3).any():
        raise ValueError(f"{path}: a face that is not a triangle")
    pick = lambda names: np.stack([v[k] for k in names], 1) if all(k in vt.names for k in names) else None  # noqa: E731
    return {"vertices": pick(("x", "y", "z")), "normals": pick(("nx", "ny", "nz")), "colors": pick(("red", "green", "blue")),
            "triangles": np.array(fa["i"], np.int32).reshape(-1, 3)}


def read_obj(path: str):
    """A Wavefront OBJ's `v` and `f` records as a dict like read_mesh_ply's (normals and colours None): face corners of the forms i, i/j,
    i/j/k and i//k, negative indices counting back from the vertices read so far, polygons cut into a fan; every other record is ignored"""
    v, t = [], []
    with open(path, "r", errors="replace") as f:
        for no, line in enumerate(f, 1):
            w = line.split()
            if not w:
                continue
            try:
                if w[0] == "v":
                    v.append((float(w[1]), float(w[2]), float(w[3])))
                elif w[0] == "f":
                    idx = []
                    for corner in w[1:]:
                        i = int(corner.split("/")[0])
                        idx.append(i - 1 if i > 0 else len(v) + i)
                        if i == 0:
                            raise ValueError("index 0")
                    for k in range(1, len(idx) - 1):
                        t.append((idx[0], idx[k], idx[k + 1]))
            except (ValueError, IndexError):
                raise ValueError(f"{path}:{no}: cannot read `{line.strip()}`")
    return {"vertices": np.array(v, np.float32).reshape(-1, 3), "normals": None, "colors": None, "triangles": np.array(t, np.int32).reshape(-1, 3)}


def write_obj(path: str, vertices, triangles):
    """`v` and `f` records, the coordinates with the nine digits that give a float32 back"""
    with open(path, "w") as f:
        for x, y, z in np.asarray(vertices, np.float32).reshape(-1, 3).tolist():
            f.write("v %.9g %.9g %.9g\n" % (x, y, z))
        for a, b, c in np.asarray(triangles, np.int64).reshape(-1, 3).tolist():
            f.write("f %d %d %d\n" % (a + 1, b + 1, c + 1))


def shade(mesh_colors, triangles, tri, uv, front, base=(180.0, 180.0, 180.0), vertices=None, dirs=None):
    """Colours for a render of eval.TriMesh.render / raycast, on the host (off the hot path): uint8 of tri's shape + (3,).  tri, uv, front:
    the render's.  With mesh_colors ((n_vertices, 3), 0..255) the colour of a hit is (1 - u - v) Ca + u Cb + v Cc.  Without them it is `base`
    times a headlight term, |n . d| / (|n| |d|) of the face normal n = (b - a) x (c - a) and the ray's direction d -- vertices ((n_vertices,
    3)) and dirs (tri's shape + (3,), in the mesh's frame) are needed for that; without them the term is 1.  A face seen from behind (front
    False) is drawn at half the brightness.  Misses are black."""
    tri = np.asarray(tri)
    shape = tri.shape
    t = tri.reshape(-1)
    hit = t >= 0
    F = np.asarray(triangles, np.int64).reshape(-1, 3)[t[hit]]
    out = np.zeros((t.size, 3), np.float64)
    if mesh_colors is not None:
        w = np.asarray(uv, np.float64).reshape(-1, 2)[hit]
        c = np.asarray(mesh_colors, np.float64).reshape(-1, 3)
        col = (1.0 - w[:, :1] - w[:, 1:]) * c[F[:, 0]] + w[:, :1] * c[F[:, 1]] + w[:, 1:] * c[F[:, 2]]
    else:
        col = np.broadcast_to(np.asarray(base, np.float64), (len(F), 3)).copy()
        if vertices is not None and dirs is not None:
            v = np.asarray(vertices, np.float64).reshape(-1, 3)
            n = np.cross(v[F[:, 1]] - v[F[:, 0]], v[F[:, 2]] - v[F[:, 0]])
            d = np.asarray(dirs, np.float64).reshape(-1, 3)[hit]
            with np.errstate(all="ignore"):
                k = np.abs((n * d).sum(1)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(d, axis=1))
            col *= np.nan_to_num(k)[:, None]
    col = np.where(np.asarray(front, bool).reshape(-1)[hit][:, None], col, 0.5 * col)
    out[hit] = col
    return np.clip(np.rint(out), 0, 255).astype(np.uint8).reshape(shape + (3,))


def camera_dirs(W: int, H: int, fx: float, fy: float, cx: float, cy: float, mesh_from_cam=None) -> np.ndarray:
    """(H, W, 3) float64: the directions of mf_trimesh_render_dev's pixel rays, turned into the mesh's frame by mesh_from_cam -- for shade()"""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1)
    return d if mesh_from_cam is None else d @ np.asarray(mesh_from_cam, np.float64)[:3, :3].T


def score_views(trimesh, vertices, triangles, colors, seq: str, poses: str, cal=None, stride: int = 1, max_dt: float = 0.02, time_scale: float = 1e-6):
    """The mesh of `trimesh` (eval.TriMesh; vertices, triangles, colors: what it was built from) rendered from the pose of every stride-th
    frame of the sequence `seq` (a directory or a .klg) and scored against that frame with eval.ViewScorer.add: coverage, depth L1, PSNR and
    SSIM.  poses: a TUM file, camera -> the mesh's frame, its stamps the frames' times time_scale (mf_export_poses' and meshseq's scale).
    cal: (fx, fy, cx, cy); default: calibration.txt of the sequence.  Where the sequence has masks, a pixel is counted in the group of its
    mask value (0: the static scene; values above 63 nowhere), so a scene's mesh is scored on the scene's pixels (group 0) apart from
    those a masked object covers.  Returns {"summary", "groups", "frames", "frames_skipped"}: ViewScorer.result()'s, without the counters."""
    from .eval import ViewScorer, _clean, associate, read_tum
    from .io.readers import load_calibration, open_log
    reader = open_log(seq)
    if cal is None:
        if getattr(reader, "calibrationFile", None) is None:
            raise ValueError(f"{seq} holds no calibration.txt: give --cal")
        cal = load_calibration(reader.calibrationFile)
    fx, fy, cx, cy = (float(v) for v in cal[:4])
    stamps, T = read_tum(poses)
    times = np.asarray(reader.timestamps(), np.float64)
    chosen = np.arange(0, len(times), max(1, int(stride)))
    pairs = associate(times[chosen] * time_scale, stamps, max_dt)
    if len(pairs) == 0:
        raise ValueError(f"none of the frames of {seq} has a pose in {poses}")
    pose_of = {int(chosen[i]): int(j) for i, j in pairs}
    scorer = ViewScorer()
    frames = (reader.load(k) for k in sorted(pose_of)) if hasattr(reader, "load") else (f for f in reader if f.index in pose_of)
    for f in frames:
        H, W = f.depth.shape
        M = T[pose_of[f.index]]
        depth, tri, uv, front = trimesh.render(W, H, fx, fy, cx, cy, M)
        rgb = shade(colors, triangles, tri, uv, front, vertices=vertices, dirs=camera_dirs(W, H, fx, fy, cx, cy, M))
        rgba = np.concatenate([rgb, np.where(tri >= 0, 255, 0).astype(np.uint8)[..., None]], -1)
        scorer.add(rgba, depth, f.rgb, f.depth, group=f.mask)
    res = scorer.result()
    return _clean({"summary": res["summary"], "groups": res["groups"], "frames": res["frames"], "frames_skipped": int(len(chosen) - len(pairs))})


def read_triangle_mesh(path: str):
    """read_mesh_ply for .ply, read_obj for .obj (by the extension, in any case)"""
    ext = path.rsplit(".", 1)[-1].lower() if "." in path else ""
    if ext == "ply":
        return read_mesh_ply(path)
    if ext == "obj":
        return read_obj(path)
    raise ValueError(f"{path}: a triangle mesh is read from .ply or .obj")


def read_cloud_ply(path: str):
    """(points, normals, colours or None) of a cloud as mf_save_ply writes it; the normals are required"""
    from .eval import read_ply
    pts, nrm = read_ply(path, normals=True)
    if nrm is None:
        raise ValueError(f"{path} has no normals (nx ny nz): estimate them first (python -m maskfusion_amd.eval --estimate-normals)")
    col = None
    try:
        col = read_ply_colors(path, len(pts))
    except ValueError:
        pass
    return pts, nrm, col


def read_ply_colors(path: str, n: int):
    """red green blue of a binary little-endian PLY's vertex element as (n, 3) float32; ValueError when there are none"""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header")
    at = raw.index(b"\n", end) + 1
    types = {"float": "<f4", "float32": "<f4", "double": "<f8", "uchar": "u1", "uint8": "u1", "char": "i1", "int": "<i4", "uint": "<u4", "short": "<i2",
             "ushort": "<u2", "int32": "<i4", "float64": "<f8"}
    props, first = [], None
    for line in raw[:end].decode("ascii", "replace").splitlines():
        w = line.split()
        if w[:1] == ["format"] and w[1] != "binary_little_endian":
            raise ValueError("colours are read from binary little-endian files only")
        if w[:1] == ["element"]:
            if first is not None:
                break
            first = w[1]
        elif w[:1] == ["property"] and first == "vertex":
            if w[1] == "list" or w[1] not in types:
                raise ValueError("unsupported vertex property")
            props.append((w[2], types[w[1]]))
    names = [p[0] for p in props]
    if not all(k in names for k in ("red", "green", "blue")):
        raise ValueError("no colours")
    v = np.frombuffer(raw, np.dtype(props), n, at)
    return np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.float32)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m maskfusion_amd.mesh", description="Mesh an exported surfel cloud (cloud-<id>.ply) on the GPU; "
                                 "score a mesh's renders against a sequence.")
    ap.add_argument("--cloud", help="a PLY cloud with normals, as -em / mf_save_ply writes it")
    ap.add_argument("--mesh", metavar="FILE", help="with --views, in place of --cloud: an existing triangle mesh (.ply or .obj) to render")
    ap.add_argument("--voxel", type=float, help="edge of a lattice cell in the cloud's unit (metres)")
    ap.add_argument("--support", type=float, default=None, help="radius of the distance field's weights (default 2.5 voxel; voxel .. 8 voxel)")
    ap.add_argument("--min-neighbours", type=int, default=3, help="points a lattice corner needs within the support (default 3)")
    ap.add_argument("-o", "--output", help="the mesh, a binary PLY")
    ap.add_argument("--fidelity", action="store_true", help="add cloud_to_mesh to the JSON line: the exact distances from the input points to "
                    "the mesh just written (radius: the support)")
    ap.add_argument("--views", metavar="SEQ", help="a sequence (a directory or a .klg): adds mesh_views to the JSON line -- the mesh rendered by "
                    "GPU ray casting from every frame's pose against the sensor's frame: coverage, depth L1, PSNR, SSIM")
    ap.add_argument("--poses", metavar="FILE", help="with --views: TUM file, camera -> the mesh's frame, stamped with the frames' times (x 1e-6, as "
                    "poses-<id>.txt and meshseq's groundtruth.txt are)")
    ap.add_argument("--cal", metavar="FILE", help="with --views: fx fy cx cy (default: the sequence's calibration.txt)")
    ap.add_argument("--stride", type=int, default=1, help="with --views: every S-th frame (default 1)")
    ap.add_argument("--view-cell", type=float, default=None, help="with --views: the ray caster's cell (default: the voxel, or for --mesh the "
                    "mesh's largest extent / 256)")
    a = ap.parse_args(argv)
    if (a.cloud is None) == (a.mesh is None):
        ap.error("give --cloud, or --mesh with --views")
    if a.mesh is not None and (a.views is None or a.fidelity or a.output or a.voxel is not None):
        ap.error("--mesh goes with --views and takes no --voxel, -o or --fidelity")
    if a.cloud is not None and (a.voxel is None or a.output is None):
        ap.error("--cloud needs --voxel and -o")
    if (a.views is None) != (a.poses is None):
        ap.error("--views and --poses go together")
    if a.views is None and (a.cal is not None or a.stride != 1 or a.view_cell is not None):
        ap.error("--cal, --stride and --view-cell need --views")
    if a.stride < 1 or (a.view_cell is not None and not (math.isfinite(a.view_cell) and a.view_cell > 0)):
        ap.error("--stride takes at least 1, --view-cell a positive length")
    try:
        if a.mesh is not None:
            m = read_triangle_mesh(a.mesh)
            v, n, c, t = m["vertices"], m["normals"], m["colors"], m["triangles"]
            info = {"mesh": a.mesh, "vertices": int(len(v)), "triangles": int(len(t))}
        else:
            pts, nrm, col = read_cloud_ply(a.cloud)
    except (OSError, ValueError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    if a.mesh is None:
        v, n, c, t = mesh_cloud(pts, nrm, col, voxel=a.voxel, support=a.support, min_neighbours=a.min_neighbours)
        write_mesh_ply(a.output, v, n, c, t)
        support = a.support if a.support is not None else 2.5 * a.voxel
        info = {"points": int(len(pts)), "vertices": int(len(v)), "triangles": int(len(t)), "voxel": a.voxel, "support": support, "output": a.output}
        if a.fidelity:
            from .eval import TriMesh, cloud_stats
            with TriMesh(v, t, support / 2) as tm:
                info["cloud_to_mesh"] = cloud_stats(tm.distance(pts, support)[0], support, (a.voxel / 4, a.voxel / 2, a.voxel))
    if a.views:
        from .eval import TriMesh
        from .io.readers import load_calibration
        cell = a.view_cell if a.view_cell is not None else a.voxel
        if cell is None:
            fin = v[np.isfinite(v).all(1)] if len(v) else v
            cell = max(float((fin.max(0) - fin.min(0)).max()) / 256.0, 1e-6) if len(fin) else 1.0
        try:
            with TriMesh(v, t, cell) as tm:
                info["mesh_views"] = score_views(tm, v, t, c, a.views, a.poses, load_calibration(a.cal) if a.cal else None, a.stride)
        except (OSError, ValueError, EOFError) as e:
            print(f"error: --views: {e}", file=sys.stderr)
            return 2
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
