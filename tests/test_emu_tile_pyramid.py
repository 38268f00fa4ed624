"""The tile pass's pyramid epilogue, its fix-up launch and the frame pyramid beside the tile pass: LOGIC and indexing on every CPU run -- the switch
combinations and the mid-stream flip of the fill-in decision of tests/test_gpu_tile_pyramid.py (its cases 1 and 2) against the product's kernels
executed on the CPU (tests/hipcpu, the plain build), at the image size tests/test_emu_smoke.py uses.  The same assertions the MI355X run makes (not
its contraction: the CPU build rounds every operation on its own); in a subprocess, so that the emulated library never enters this process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_tile_pyramid_switches_and_fill_in_flip():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_tile_pyramid.py"), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "every_switch_combination or flips_in_mid_stream"],
                       capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "9 passed" in r.stdout, r.stdout[-1000:]
