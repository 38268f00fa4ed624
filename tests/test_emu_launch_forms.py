"""The launch forms a frame size selects (tests/test_gpu_launch_forms.py): LOGIC and indexing on every CPU run -- which k_icp_iter form each size
gets, one ICP step per form with its tail / upper-slot variants, the SO(3) pre-alignment at a partial last workgroup and above one pixel per
thread, preprocessing at sizes with partial tiles, and three frames of the 424x240 pipeline -- against the product's kernels executed on the CPU
(tests/hipcpu, the plain build).  The same assertions the MI355X run makes (not the hardware's scalar branches, LDS traffic, wave shuffles or
contraction: the CPU build rounds every operation on its own); in a subprocess, so that the emulated library never enters this process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_launch_forms():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1", MF_LAUNCH_FORM_FRAMES="3")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_launch_forms.py"), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not rgbd-so3 and not 416x296-icp"],
                       capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "28 passed" in r.stdout, r.stdout[-1000:]
