"""The hypothesis search (tests/test_gpu_pose_ransac.py: planted motions at every size the kernels branch on, edge cases, argument errors, the
Python side and register_global on it) and the recognition of a returning object (tests/test_gpu_redetect.py) on every CPU run: the same
assertions the MI355X run makes, against the product's kernels executed on the CPU (tests/hipcpu, the plain build) -- the LOGIC, indexing and
fp64 operation order of mf_register.hip, not the hardware's atomics.  In a subprocess, so that the emulated library never enters this process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_pose_ransac_and_redetection():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_pose_ransac.py"), os.path.join(ROOT, "tests", "test_gpu_redetect.py"),
                        "-q", "-n", "0", "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "29 passed" in r.stdout, r.stdout[-1000:]
