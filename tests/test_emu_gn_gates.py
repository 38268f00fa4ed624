"""The crafted correspondence-gate cases (tests/test_gpu_gn_gates.py: one candidate pixel per case, the minefields through the four kernels that
inline the per-pixel functions, the slab culling's margin, the photometric cases and gate images, the weight's epsilon, the refused thresholds)
on every CPU run: the same assertions the MI355X run makes, against the product's kernels executed on the CPU (tests/hipcpu, the plain build) --
the LOGIC of the gates, the launch forms' indexing and the slab culling, not the hardware's conversions and reductions.  In a subprocess, so
that the emulated library never enters this process.  Measured: the 123 cases take 12 s of wall time on one process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_gn_gates():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_gn_gates.py"), "-q", "-n", "0", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "123 passed" in r.stdout, r.stdout[-1000:]
