"""The host half of rpt_particles_* on a CPU: tests/host/particles_harness.cpp drives the real rpt_amd/csrc/rpt_particles.cpp
(malloc-backed HIP stubs, tests/host/hip_stubs.h) through a handle's life cycle -- bad parameters, a failed allocation, the cut of a
2,500-step sequence into launches of at most 256 steps with the right last step, the event that orders a handle's calls, the check
order, a set_state issued while an integrate is queued -- with stubs of the launchers that touch every byte the kernels would.

  * as a program of its own under AddressSanitizer + UBSan (g++ -O1) and plain (g++ -O1): no failure, no report, the same output.

No GPU; nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "particles_harness.cpp")
COMMON = ["-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")]


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + flags + COMMON + [SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(p.stdout[-6000:])
    assert "FAILED" not in p.stdout, "\n".join(l for l in p.stdout.splitlines() if "FAILED" in l)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-2000:]
    return p.stdout


def test_handle_life_cycle_launch_split_and_check_order(tmp_path):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    san = _build_and_run(tmp_path, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    plain = _build_and_run(tmp_path, "plain", ["-O1"])
    assert san == plain
    lines = san.splitlines()
    assert len(lines) == 27 and all(l.endswith(": ok") for l in lines[:-1])
    assert lines[-1] == "launches=4109 waits=4 records=5 failures=0", lines[-1]
