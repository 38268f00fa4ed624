"""The crafted label-stage cases (tests/test_gpu_label_edges.py: components, sweeps, votes and decisions, closing, table overflow, random sweep)
on every CPU run: the same assertions the MI355X run makes, against the product's kernels executed on the CPU (tests/hipcpu, the plain build) --
the LOGIC and indexing of the 16 kernels of mf_labels_gpu.hip, not the hardware's ballots, shuffles and atomics.  In a subprocess, so that the
emulated library never enters this process.  Measured: the 312 cases take 20 s of wall time on one process (the two emulated 320x240 cases of
tests/test_gpu_labels.py take 3 s); half of it is LabelsScratch::init clearing its two 32 MB vote tables per call."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_label_edges():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_label_edges.py"), "-q", "-n", "0", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "312 passed" in r.stdout, r.stdout[-1000:]
