"""CPU twin of the generator half of tests/test_gpu_isres_gated.py: the same tests over the emulated device layer
(oracle/libnlopt_amd_emu.so through tests/_emu_plugin.py, in a pytest process of its own).  oracle/emu_device.c keeps a copy of its own of
nla_rankbits_gate_target — the formula the emulated ranking pipeline refuses to run without — and its nla_k_mt_rankbits_gated states the
generator's contract the slow way: all bits, then every gate at its target and the ticket moved by the number of segments.  Checked here,
on the table of the GPU file: that copy of the formula against the brute-force count of segments, and gate[c] == target(c),
ticket == segments, bits == the serial generator's after the emulated launch (one waves_per_cu, which the emulation ignores)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so")


def test_gate_targets_and_gated_generator_over_the_emulated_device():
    assert os.path.exists(EMU), "the emulated library is not built (tests/conftest.py builds it)"
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "tests"), NLA_TEST_EMU_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-p", "_emu_plugin", os.path.join(ROOT, "tests", "test_gpu_isres_gated.py"),
                        "-m", "gpu", "-q", "-p", "no:cacheprovider", "-x", "--tb=short", "-k",
                        "gate_target or (generator_alone and wpc8)"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    # 7 launches of the generator (the table and the boundary case) and the formula on every one of those and on the boundary layouts
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    npassed = int(tail.split(" passed")[0].split()[-1])
    assert npassed >= 7 + 7, tail
