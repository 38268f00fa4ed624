"""The deferred prediction's LOGIC on every CPU run: the switch combinations and the settle points of tests/test_gpu_deferred_predict.py (its cases
1 and 2) against the product's kernels executed on the CPU (tests/hipcpu, the plain build), at the image size tests/test_emu_smoke.py uses.  The same
assertions the MI355X run makes; in a subprocess, so that the emulated library never enters this process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_deferred_prediction_switches_and_settle_points():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_deferred_predict.py"), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "every_switch_combination or settles_the_pending_prediction"],
                       capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "17 passed" in r.stdout, r.stdout[-1000:]
