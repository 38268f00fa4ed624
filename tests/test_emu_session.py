"""Sessions on every CPU run: the single-model continuation (the save meets a pending prediction), the two-object continuation saved in the frame
of the spawn, the refusals of malformed files and the failed save of tests/test_gpu_session.py against the product's kernels executed on the CPU
(tests/hipcpu, the plain build), at the image size tests/test_emu_smoke.py uses.  The same assertions the MI355X run makes; in a subprocess, so that the
emulated library never enters this process."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_session_continuations_and_refusals():
    env = dict(os.environ, MF_EMU="1", MF_NO_PREBUILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_session.py"), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_continuation_single_model[icp-defer1] or test_continuation_with_objects[spawn] or malformed_files or failed_save"],
                       capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout, r.stdout[-1000:]
