"""Builds libmaskfusion_amd.so (HIP, gfx950 only) in-tree with hipcc.  No CPU fallback exists."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmaskfusion_amd.so")
SOURCES = ["mf_preproc.hip", "mf_odometry.hip", "mf_model_pyramid.hip", "mf_rgbd.hip", "mf_surfel.hip", "mf_splat.hip", "mf_segment.hip", "mf_labels.hip", "mf_labels_gpu.hip", "mf_render.hip", "mf_eval.hip", "mf_eval_image.hip", "mf_eval_visibility.hip", "mf_mesh.hip", "mf_eval_trimesh.hip", "mf_trimesh_ray.hip", "mf_register.hip", "mf_merge.hip", "mf_session.hip", "mf_context.hip"]
HEADERS = ["mf_internal.h", "mf_device.h", "mf_labels.h", os.path.join("..", "..", "include", "maskfusion_amd.h"), "mf_rgbd_device.h", "mf_walk.h", "mf_sprite_device.h", "mf_cloud_grid.h", "mf_trimesh.h",
           "mf_bilateral_device.h", "mf_frame_pyramid_device.h", "mf_model_pyramid_device.h", "mf_gn_device.h",
           "mf_frame.inl", "mf_model_api.inl", "mf_params.inl", "mf_ktest.inl", "mf_render.inl", "mf_eval.inl", "mf_session.inl"]   # (the .inl files are parts of mf_context.hip)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]
# per-file additions.  mf_odometry: the SLP vectoriser pairs the 28 upper-triangle products of the ICP row into v_pk_fma_f32 and then
# spends more v_mov_b32 on assembling the operand pairs than it saves (k_icp_iter<512>: 2643 -> 2432 instructions, 589 -> 286 moves)
# mf_model_pyramid: its kernels were part of mf_odometry.hip and keep the flag they were tuned and pinned under (DESIGN.md finding F10)
# mf_eval: no contraction anywhere, so that the nearest-neighbour distances are bit-identical to an fp32 numpy brute force
# mf_eval_image: no contraction either, so that the view scores' fp64 arithmetic is rounded operation by operation as the header gives it
# mf_eval_visibility: nor here, so that a point's fp32 projection has the bits of the header's operation-by-operation statement
# mf_mesh: the grid's rounding argument and the header's operation-by-operation definition of the field, as mf_eval
# mf_eval_trimesh: the header's operation-by-operation fp64 point-to-triangle distance, which the tests compare bit for bit
# mf_trimesh_ray: the header's operation-by-operation fp64 ray-triangle test, compared bit for bit as well
# mf_register: the header's operation-by-operation fp64 fit and score of a triple, compared bit for bit too
# mf_merge: the header's operation-by-operation fp32 merge rule and the grid's rounding argument, compared bit for bit as well
# mf_session: self-contained like them (integer digests and copies: no floating-point arithmetic to contract)
FILE_FLAGS = {"mf_odometry.hip": ["-fno-slp-vectorize"], "mf_model_pyramid.hip": ["-fno-slp-vectorize"], "mf_eval.hip": ["-ffp-contract=off"], "mf_eval_image.hip": ["-ffp-contract=off"],
              "mf_eval_visibility.hip": ["-ffp-contract=off"], "mf_mesh.hip": ["-ffp-contract=off"], "mf_eval_trimesh.hip": ["-ffp-contract=off"],
              "mf_trimesh_ray.hip": ["-ffp-contract=off"], "mf_register.hip": ["-ffp-contract=off"], "mf_merge.hip": ["-ffp-contract=off"],
              "mf_session.hip": ["-ffp-contract=off"]}


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the MI355X path cannot be built (there is no CPU fallback)")


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force: bool = False, verbose: bool = False, extra_flags=()) -> str:
    if not (force or _stale()):
        return LIB
    hipcc = _hipcc()
    objs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        cmd = [hipcc, *FLAGS, *FILE_FLAGS.get(src, []), *extra_flags, "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        objs.append(obj)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
