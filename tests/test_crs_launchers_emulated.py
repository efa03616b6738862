"""CPU twin of tests/test_gpu_crs_launchers.py: that module over the emulated device layer (oracle/libnlopt_amd_emu.so through
tests/_emu_plugin.py, in a pytest process of its own — the package holds one library per process).  The HIP kernels are not run here.
What this proves without a GPU:
  - the module's expectations — whole-row statements sliced in numpy, "commit on a host copy, then the statement", the pick-list
    assertions that every named situation occurs — agree with the emulation's independent C statements of the launchers' contracts
    (oracle/emu_device.c: the column launchers through the column statements, the fused commit as commit-then-advance, the lean
    window launch, obj = -2, the refusals), so a failure on the GPU points at a kernel and not at the test;
  - its harness (ring layout, lists as host arrays, pinned buffers, the ctypes signatures of nlopt_amd/__init__.py) is sound.
The comparisons "bit-identical to the pointer form / to nla_k_crs_finish" run here too; they hold trivially.  No case is skipped."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so")


@pytest.mark.skipif(not os.path.exists(EMU), reason="the emulated library is not built")
def test_crs_launcher_tests_over_the_emulated_device():
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests"), NLA_TEST_EMU_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-p", "_emu_plugin", os.path.join(ROOT, "tests", "test_gpu_crs_launchers.py"), "-m", "gpu", "-q",
                        "-p", "no:cacheprovider", "-x", "--tb=short"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and " skipped" not in tail and " deselected" not in tail, tail
