"""The host half of RPT_TEMPORAL_CLIP and rpt_temporal_set_clip on a CPU: tests/host/temporal_clip_harness.cpp drives the real
rpt_amd/csrc/rpt_capi.cpp (malloc-backed HIP stubs, tests/host/hip_stubs.h) with a stub of the accumulation kernel that records its
arguments: the setter's refusals in their order and before the handle, the defaults when it was never called, the three values and
the flag arriving in the kernel's arguments through all three entry points and only with the flag, their persistence over calls and
over a reset, a refused set leaving them, a refused call launching nothing, and the record swap staying as
tests/host/temporal_harness.cpp observes it.

  * as a program of its own under AddressSanitizer + UBSan (g++ -O1) and plain (g++ -O1): no failure, no report, the same output.

No GPU, no oracle; nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "temporal_clip_harness.cpp")
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


def test_clip_settings_are_checked_kept_and_passed_to_the_kernel(tmp_path):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    san = _build_and_run(tmp_path, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    plain = _build_and_run(tmp_path, "plain", ["-O1"])
    assert san == plain
    lines = san.splitlines()
    assert len(lines) == 17 and all(l.endswith(": ok") for l in lines[:-1])
    assert lines[-1].endswith("failures=0"), lines[-1]
