"""Mesh rendering on every CPU run: the icosphere, the mixed-size mesh and render == raycast of tests/test_gpu_raycast.py against the numpy
restatement through the product's kernels EXECUTED ON THE CPU (tests/hipcpu), in one subprocess as tests/test_emu_trimesh.py runs its tests:
nothing of the emulator leaks into this process.  The bit-for-bit claim about the hardware rests on the -m gpu run of the same tests."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_raycast_and_render_on_the_cpu_executed_kernels():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    tests = ["test_gpu_raycast.py::test_icosphere_is_the_restatements", "test_gpu_raycast.py::test_mixed_sizes_are_the_restatements",
             "test_gpu_raycast.py::test_render_is_raycast_on_the_pinhole_rays"]
    r = subprocess.run([sys.executable, "-m", "pytest", *[os.path.join(ROOT, "tests", t) for t in tests], "-q", "-m", "gpu", "-n", "0", "-x", "-s",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "3 passed" in r.stdout and "triangles that differ: 0" in r.stdout and "t: 0 not bit-equal" in r.stdout, tail
