"""CPU twin of tests/test_gpu_isres_evolve.py: that module over the emulated device layer (oracle/libnlopt_amd_emu.so through
tests/_emu_plugin.py, in a pytest process of its own — the package holds one library per process), with NLA_EMU_EVOLVE2 set.
The HIP kernels are not run here.  What this proves without a GPU:
  - the module's numpy.longdouble reference equals the emulation's independent C statement of the evolve contract
    (oracle/emu_device.c: nla_k_isres_evolve) — deviate positions exactly, X and S within the module's bounds, the run-out rule;
  - its harness plays the round / refill / hand-over protocol of isres_driver.c correctly: the emulated rounds force hand-overs
    (a fixed function of the individual's index) and run out of deviates in the middle of a round.
The module skips only what the emulation defines away (that a hand-over happened, state[11], parent_mu, supported())."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so")


@pytest.mark.skipif(not os.path.exists(EMU), reason="the emulated library is not built")
def test_evolve_kernel_tests_over_the_emulated_device():
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests"), NLA_TEST_EMU_DEVICE="1", NLA_EMU_EVOLVE2="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-p", "_emu_plugin", os.path.join(ROOT, "tests", "test_gpu_isres_evolve.py"), "-m", "gpu", "-q",
                        "-p", "no:cacheprovider", "-x", "--tb=short"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail, tail
