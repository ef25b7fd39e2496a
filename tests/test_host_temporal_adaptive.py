"""The host half of adaptive sampling over a sequence on a CPU: tests/host/temporal_adaptive_harness.cpp drives the real
rpt_amd/csrc/rpt_capi.cpp (malloc-backed HIP stubs, tests/host/hip_stubs.h) with stubs of the loop's kernels that log their
arguments: the order of the three entry points' refusals, all before any device call; a preview that consumes neither the motion
table nor the frame count, is ordered through the accumulator's event and leaves the records unswapped; a host table uploaded once
however many calls read it; the loop's call sequence round by round and the life of its active list; the loop leaving the accumulator
as it found it.

  * as a program of its own under AddressSanitizer + UBSan (g++ -O1) and plain (g++ -O1): no failure, no report, the same output.

No GPU, no oracle; nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "temporal_adaptive_harness.cpp")
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


def test_previews_consume_nothing_and_the_loop_calls_its_kernels_in_order(tmp_path):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    san = _build_and_run(tmp_path, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    plain = _build_and_run(tmp_path, "plain", ["-O1"])
    assert san == plain
    checks = [l for l in san.splitlines() if not l.startswith("  ")]
    assert len(checks) == 14 and all(l.endswith(": ok") for l in checks[:-1])
    assert checks[-1] == "failures=0", checks[-1]
