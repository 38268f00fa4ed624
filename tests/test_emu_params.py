"""The table of the parameter keys on every CPU run: tests/test_gpu_params.py -- defaults, round trips, refusals, access, the taps after three
frames -- against the product's host code and kernels executed on the CPU (tests/hipcpu, the plain build).  The same assertions the MI355X run
makes; in a subprocess, so that the emulated library never enters this process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_parameter_table():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_params.py"), "-q", "-x", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 passed" in r.stdout, r.stdout[-1000:]
