"""MaskFusion::renderView of the C++ facade (tests/cpp/render_main.cpp) against MaskFusion.renderView of the Python mirror: same library,
same stream, same view -> the same bytes."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_render import CLS, PALETTE, W, H, F, _camera_view, _context, _frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_render_matches_python(hip, tmp_path):
    _, frames = _frames(6)
    m = _context()
    for k, (rgb, depth, mask) in enumerate(frames):
        m.processFrame(rgb, depth, mask=mask, classIDs=CLS, timestamp=k)
    v = _camera_view(m)
    v.background_color_type, v.object_color_type = 2, 4
    rgba, dep, mod = m.renderView(v, palette=PALETTE, depth=True, models=True)
    n_models = len(m.getModels())
    m.close()
    blob = tmp_path / "frames.bin"
    with open(blob, "wb") as f:
        for rgb, depth, mask in frames:
            f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
            f.write(np.ascontiguousarray(depth, np.float32).tobytes())
            f.write(np.ascontiguousarray(mask, np.uint8).tobytes())
    lib = hip._name if os.environ.get("MF_EMU") == "1" else os.path.join(ROOT, "maskfusion_amd", "libmaskfusion_amd.so")
    exe = os.path.join(str(tmp_path), "render_main")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "render_main.cpp"),
           "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, str(W), str(H), str(F), str(F), str(W / 2.0), str(H / 2.0), str(len(frames)), str(blob), str(out)], capture_output=True,
                       text=True, timeout=1800)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert f"models {n_models}" in r.stdout
    raw = open(out, "rb").read()
    P = W * H
    c_rgba = np.frombuffer(raw[:4 * P], np.uint8).reshape(H, W, 4)
    c_dep = np.frombuffer(raw[4 * P:8 * P], np.float32).reshape(H, W)
    c_mod = np.frombuffer(raw[8 * P:12 * P], np.int32).reshape(H, W)
    assert (mod > 0).any() and (mod == 0).any()
    assert np.array_equal(c_rgba, rgba) and np.array_equal(c_dep, dep) and np.array_equal(c_mod, mod)
