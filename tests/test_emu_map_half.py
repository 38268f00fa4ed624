"""The two switches of the map half ("cleanTapGroup", "maskFreeClean"): LOGIC and indexing on every CPU run -- the switch
combinations over the stream and the crafted windows of tests/test_gpu_map_half.py (its groups 1 and 2) against the product's kernels executed on
the CPU (tests/hipcpu, the plain build).  The same assertions the MI355X run makes (not its contraction: the CPU build rounds every operation on its
own); in a subprocess, so that the emulated library never enters this process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_map_half_switches_and_crafted_windows():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_map_half.py"), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "every_switch_combination or crafted_windows"],
                       capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "18 passed" in r.stdout, r.stdout[-1000:]
