"""One committed scene through mixed call sequences, on a CPU: tests/host/sequence_harness.cpp drives the real
rpt_amd/csrc/rpt_capi.cpp (malloc-backed HIP stubs, tests/host/hip_stubs.h) through renders of changing sizes and shards, tile-list
renders and feature passes, in fp32 and in the reference-epsilon mode, on one stream, on two streams in turn, and through the host
entry point while a device call is queued on another stream.  The stubs keep a model of what the device still has in flight (the
harness's header comment): a copy or memset into memory a queued launch was handed, two launches in flight on one slab or work
counter, a launch whose tile ids are not rpt_shard_tiles of its own call, a slab too small for its items, a sharded frame that was
not cleared -- each is a finding, printed, and the exit code is 1.

  * under AddressSanitizer + UBSan (g++ -O1) and plain (g++ -O1): no finding, no report, the same output.

The in-place rewrite of the scene's one tile list on a change of frame (1,944 findings, all
of them that rewrite, before prepare_render kept one list per frame)
is what this pins; tests/test_gpu_call_sequences.py is its counterpart on the device.  No GPU, no oracle."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "sequence_harness.cpp")
COMMON = ["-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")]
GROUPS = ("sizes", "shards", "tile list", "features", "many frames")
POLICIES = ("one stream", "two streams in turn", "a stream and the host entry point in turn")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + flags + COMMON + [SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(p.stdout[-6000:])
    assert "FINDING" not in p.stdout, "\n".join(l for l in p.stdout.splitlines() if l.startswith("FINDING"))[:4000]
    assert p.returncode == 0, p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    return p.stdout


@pytest.mark.timeout(600)
def test_no_call_sequence_touches_what_a_queued_launch_was_handed(tmp_path):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    san = _build_and_run(tmp_path, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    plain = _build_and_run(tmp_path, "plain", ["-O1"])
    assert san == plain
    lines = san.splitlines()
    for mode in ("fp32", "epsilon"):               # every sequence ran, and launched: a render and a resolve (or two feature kernels) per call
        for g, calls in zip(GROUPS, (5, 3, 4, 5, 20)):
            for p in POLICIES:
                assert f"{mode} {g}, {p}: {2 * calls} launches, 0 findings" in lines, (mode, g, p)
    total = 2 * 3 * 2 * (5 + 3 + 4 + 5 + 20)
    assert lines[-1].startswith(f"launches={total} ") and lines[-1].endswith(" findings=0 still in flight=0"), lines[-1]
