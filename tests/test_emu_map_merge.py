"""Map merging (tests/test_gpu_map_merge.py: the kernel against the restatement at every size and edge; tests/test_gpu_merge_models.py:
mf_model_merge_map, re-detection that keeps the new map, the join of two sessions) on every CPU run: the same assertions the MI355X run makes,
against the product's kernels executed on the CPU (tests/hipcpu, the plain build) -- the LOGIC, indexing and fp32 operation order of
mf_merge.hip, not the hardware's atomics.  In a subprocess, so that the emulated library never enters this process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_map_merge():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_map_merge.py"), os.path.join(ROOT, "tests", "test_gpu_merge_models.py"),
                        "-q", "-n", "0", "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "36 passed" in r.stdout, r.stdout[-1000:]
