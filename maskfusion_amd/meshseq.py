"""An RGB-D + mask sequence rendered from triangle meshes by GPU ray casting (eval.TriMesh.render: mf_trimesh_render_dev, kernels:
csrc/mf_trimesh_ray.hip; the definition: include/maskfusion_amd.h; DESIGN.md "Mesh rendering").

    python -m maskfusion_amd.meshseq --mesh scene.obj --object part.ply:CLASS[:traj.txt] ... --poses cam.txt
        [--cal FILE] [--size WxH] [--max-depth D] [--noise SEED] [--depth png|exr] -o seq/

--mesh is the static scene, every --object a mesh of its own with the class id its mask is given and, optionally, a TUM trajectory of the
object in the world (T_world_obj; taken by the nearest time stamp; none: the object stands where its mesh does).  --poses is the camera's
TUM trajectory (T_world_cam): one frame per line.  Each mesh is built once (one TriMesh); per frame each is rendered with mesh_from_cam =
inv(T_world_obj(t)) T_world_cam(t) -- only the ray transform changes when an object moves -- and the renders are composited by the least
depth on the host: an object wins an exact tie over the scene, a lower object number over a higher.

The directory is what io.readers.ImageLogReader opens and `python -m maskfusion_amd.cli -dir seq/` runs: Color####.png, Depth####.png
(16-bit millimetres; --depth exr: Depth####.exr, float32 metres, nothing rounded), Mask####.png (0: the scene, k: object k) with
Mask####.txt (the objects' class ids), calibration.txt; beside them groundtruth.txt (the camera, T_world_cam) and object-<k>.txt
(T_world_obj per frame), TUM lines stamped with the frames' times as the reader stamps them, times 1e-6 -- the scale of poses-<id>.txt,
so maskfusion_amd.eval reads them with its defaults.  Colours: a mesh's vertex colours where it has them, else a base colour under a
headlight (mesh.shade)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

PALETTE = ((200, 90, 70), (80, 160, 210), (110, 190, 100), (220, 190, 80), (170, 110, 200), (90, 200, 190))
SCENE_BASE = (180, 180, 180)


def rot_to_quat(R) -> np.ndarray:
    """3 x 3 -> (qx, qy, qz, qw), qw >= 0: the branch of the largest of the four squares (Shepperd)"""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    k = int(np.argmax([R[0, 0], R[1, 1], R[2, 2], tr]))
    if k == 3:
        q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1.0 + tr])
    else:
        i, j, l = k, (k + 1) % 3, (k + 2) % 3
        q = np.zeros(4)
        q[i] = 1.0 + R[i, i] - R[j, j] - R[l, l]
        q[j] = R[i, j] + R[j, i]
        q[l] = R[i, l] + R[l, i]
        q[3] = R[l, j] - R[j, l]
    q /= np.linalg.norm(q)
    return q if q[3] >= 0 else -q


def tum_line(stamp: float, T) -> str:
    T = np.asarray(T, np.float64)
    return "%.6f %.17g %.17g %.17g %.17g %.17g %.17g %.17g" % ((stamp,) + tuple(T[:3, 3]) + tuple(rot_to_quat(T[:3, :3])))


def composite(depths):
    """depths: the scene's render first, then the objects' in their order, 0: nothing.  Returns (depth, winner): the least depth per pixel
    and whose it is (0: the scene, also where nothing was hit); an object wins an exact tie over the scene, a lower number over a higher"""
    best = np.array(depths[0], np.float32)
    winner = np.zeros(best.shape, np.uint8)
    for k in range(1, len(depths)):
        d = depths[k]
        take = (d > 0) & ((best == 0) | (d < best) | ((d == best) & (winner == 0)))
        best = np.where(take, d, best)
        winner = np.where(take, np.uint8(k), winner)
    return best, winner


class Sequence:
    """the meshes of a scene on the device and their per-frame renders; a context manager"""

    def __init__(self, scene, objects, cell=None):
        """scene: mesh.read_triangle_mesh()'s dict; objects: a list of (dict, class id, (stamps, poses) or None)"""
        from .eval import TriMesh
        self.meshes = [scene] + [o[0] for o in objects]
        self.class_ids = [0] + [int(o[1]) for o in objects]
        self.trajectories = [None] + [o[2] for o in objects]
        self.tri = []
        for m in self.meshes:
            v = np.asarray(m["vertices"], np.float32).reshape(-1, 3)
            fin = v[np.isfinite(v).all(1)]
            c = cell if cell is not None else (max(float((fin.max(0) - fin.min(0)).max()) / 128.0, 1e-6) if len(fin) else 1.0)
            self.tri.append(TriMesh(v, m["triangles"], c))

    def object_pose(self, k: int, stamp: float) -> np.ndarray:
        tr = self.trajectories[k]
        if tr is None or len(tr[0]) == 0:
            return np.eye(4)
        return tr[1][int(np.argmin(np.abs(tr[0] - stamp)))]

    def frame(self, T_world_cam, stamp, W, H, fx, fy, cx, cy, max_depth=np.inf):
        """(rgb uint8 (H, W, 3), depth float32 (H, W), mask uint8 (H, W), the objects' poses in the world)"""
        from .mesh import camera_dirs, shade
        renders, poses = [], []
        for k, t in enumerate(self.tri):
            T_obj = self.object_pose(k, stamp)
            M = np.linalg.inv(T_obj) @ np.asarray(T_world_cam, np.float64)
            renders.append((t.render(W, H, fx, fy, cx, cy, M, 0.0, max_depth), M))
            poses.append(T_obj)
        depth, winner = composite([r[0][0] for r in renders])
        rgb = np.zeros((H, W, 3), np.uint8)
        for k, ((d, tri, uv, front), M) in enumerate(renders):
            m = self.meshes[k]
            base = SCENE_BASE if k == 0 else PALETTE[(k - 1) % len(PALETTE)]
            col = shade(m.get("colors"), m["triangles"], tri, uv, front, base, vertices=m["vertices"], dirs=camera_dirs(W, H, fx, fy, cx, cy, M))
            mine = (winner == k) & (d > 0)
            rgb[mine] = col[mine]
        return rgb, depth, winner, poses[1:]

    def close(self):
        for t in self.tri:
            t.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def write_sequence(seq: "Sequence", cam_log, out: str, W: int, H: int, fx: float, fy: float, cx: float, cy: float, max_depth=np.inf, noise=None,
                   depth_format: str = "png") -> dict:
    """renders one frame per pose of cam_log (read_tum()'s pair) and writes the directory; returns what the command prints"""
    from .io.readers import ImageLogReader
    from .io.writers import write_image_dir
    from .synth import add_sensor_noise
    os.makedirs(out, exist_ok=True)
    n_obj = len(seq.tri) - 1
    gt, obj_lines = [], [[] for _ in range(n_obj)]
    hits = 0
    for i, (stamp, T) in enumerate(zip(*cam_log)):
        rgb, depth, mask, poses = seq.frame(T, stamp, W, H, fx, fy, cx, cy, max_depth)
        if noise is not None:
            depth = add_sensor_noise(depth, int(noise) + i)
        hits += int((depth > 0).sum())
        write_image_dir(out, [(rgb, depth)], masks=[mask], class_ids=[seq.class_ids], calibration=(fx, fy, cx, cy, W, H) if i == 0 else None,
                        start_index=i, depth_format=depth_format)
        t_out = int(i * 1000.0 / ImageLogReader.rateHz) * 1e-6            # the reader's stamp of frame i, on poses-<id>.txt's scale
        gt.append(tum_line(t_out, T))
        for k in range(n_obj):
            obj_lines[k].append(tum_line(t_out, poses[k]))
    with open(os.path.join(out, "groundtruth.txt"), "w") as f:
        f.write("# timestamp tx ty tz qx qy qz qw (camera -> world)\n" + "\n".join(gt) + "\n")
    for k in range(n_obj):
        with open(os.path.join(out, f"object-{k + 1}.txt"), "w") as f:
            f.write(f"# timestamp tx ty tz qx qy qz qw (object {k + 1} -> world), class {seq.class_ids[k + 1]}\n" + "\n".join(obj_lines[k]) + "\n")
    n = len(gt)
    return {"output": out, "frames": n, "width": W, "height": H, "objects": n_obj, "class_ids": seq.class_ids[1:],
            "triangles": [int(t.n_triangles) for t in seq.tri], "depth_coverage": hits / max(1, n * W * H), "depth": depth_format}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m maskfusion_amd.meshseq", description="Render an RGB-D + mask sequence from triangle meshes on the GPU.")
    ap.add_argument("--mesh", required=True, help="the static scene (.ply or .obj)")
    ap.add_argument("--object", action="append", default=[], metavar="FILE:CLASS[:TRAJ]", help="an object's mesh, the class id of its mask and, "
                    "optionally, its TUM trajectory in the world (object -> world); may be given several times: object 1, 2, ...")
    ap.add_argument("--poses", required=True, help="the camera's TUM trajectory (camera -> world): one frame per line")
    ap.add_argument("--cal", help="fx fy cx cy [w h] (default: 528 528 320 240 scaled to the size)")
    ap.add_argument("--size", default=None, metavar="WxH", help="the frames' size (default: the calibration's, else 640x480)")
    ap.add_argument("--max-depth", type=float, default=None, metavar="D", help="nothing beyond D metres is measured")
    ap.add_argument("--noise", type=int, default=None, metavar="SEED", help="synth.add_sensor_noise on every depth frame")
    ap.add_argument("--depth", choices=("png", "exr"), default="png", help="Depth####.png, 16-bit millimetres (default), or .exr, float32 metres")
    ap.add_argument("--cell", type=float, default=None, help="the ray caster's cell (default: each mesh's largest extent / 128)")
    ap.add_argument("-o", "--output", required=True, help="the sequence's directory")
    a = ap.parse_args(argv)
    from .eval import read_tum
    from .io.readers import load_calibration
    from .mesh import read_triangle_mesh
    if len(a.object) > 254:
        ap.error("at most 254 objects: a mask is one byte")
    try:
        cal = load_calibration(a.cal) if a.cal else None
        if a.size:
            W, H = (int(x) for x in a.size.lower().split("x"))
        else:
            W, H = (cal[4], cal[5]) if cal and cal[4] else (640, 480)
        if W < 1 or H < 1 or W > 16384 or H > 16384:
            raise ValueError("--size takes 1 .. 16384 per side")
        fx, fy, cx, cy = cal[:4] if cal else (528.0 * W / 640, 528.0 * H / 480, 320.0 * W / 640, 240.0 * H / 480)
        if a.max_depth is not None and not a.max_depth > 0:
            raise ValueError("--max-depth takes a positive depth")
        if a.cell is not None and not a.cell > 0:
            raise ValueError("--cell takes a positive length")
        scene = read_triangle_mesh(a.mesh)
        objects = []
        for spec in a.object:
            part = spec.split(":")
            if len(part) not in (2, 3):
                raise ValueError(f"--object {spec}: expected FILE:CLASS[:TRAJ]")
            cls = int(part[1])
            if not 0 < cls < 256:
                raise ValueError(f"--object {spec}: the class id is 1 .. 255")
            objects.append((read_triangle_mesh(part[0]), cls, read_tum(part[2]) if len(part) == 3 else None))
        cam_log = read_tum(a.poses)
        if len(cam_log[0]) == 0:
            raise ValueError(f"{a.poses} holds no pose")
    except (OSError, ValueError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    with Sequence(scene, objects, a.cell) as seq:
        info = write_sequence(seq, cam_log, a.output, W, H, fx, fy, cx, cy, np.inf if a.max_depth is None else a.max_depth, a.noise, a.depth)
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
