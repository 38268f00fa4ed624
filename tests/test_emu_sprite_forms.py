"""The sprite forms on crafted sprites (tests/test_gpu_sprite_forms.py) on every CPU run: the same assertions the MI355X run makes, against the
product's kernels executed on the CPU (tests/hipcpu, the plain build) -- the LOGIC, indexing and fp32 operation order of mf_sprite_device.h and
its four callers, not the hardware's atomics.  In a subprocess, so that the emulated library never enters this process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_sprite_forms():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_sprite_forms.py"), "-q", "-n", "0", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "7 passed" in r.stdout, r.stdout[-1000:]
