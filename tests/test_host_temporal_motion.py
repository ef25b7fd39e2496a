"""The host half of rpt_temporal_set_motion* on a CPU: tests/host/temporal_motion_harness.cpp drives the real
rpt_amd/csrc/rpt_capi.cpp (malloc-backed HIP stubs, tests/host/hip_stubs.h) with a stub of the accumulation kernel that reads every
byte of the motion table it is given: the table reaches the next launch and no later one (the first frame's included), a refused
call leaves it, a reset drops it, a second set replaces the first, NULL / 0 clears, a value that is not finite is refused before any
device call, a growing table reallocates without a leak, the upload follows the wait for the predecessor's event on the consuming
call's stream and reads the accumulator's own copy, the device variant passes the caller's pointer through, and the record swap and
the event waits stay as tests/host/temporal_harness.cpp observes them.

  * as a program of its own under AddressSanitizer + UBSan (g++ -O1) and plain (g++ -O1): no failure, no report, the same output.

No GPU, no oracle; nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "temporal_motion_harness.cpp")
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


def test_motion_table_is_one_shot_ordered_and_owned(tmp_path):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    san = _build_and_run(tmp_path, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    plain = _build_and_run(tmp_path, "plain", ["-O1"])
    assert san == plain
    lines = san.splitlines()
    assert len(lines) == 21 and all(l.endswith(": ok") for l in lines[:-1])
    assert lines[-1].endswith("failures=0"), lines[-1]
