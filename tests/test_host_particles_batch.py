"""The host half of rpt_particles_batch_* on a CPU: tests/host/particles_batch_harness.cpp drives the real
rpt_amd/csrc/rpt_particles.cpp (malloc-backed HIP stubs, tests/host/hip_stubs.h) through a batch's life cycle -- every refusal in its
stated order, a failed allocation at each allocation, the launch rule at R = 4 for 1, 4, 5, 9 and 1,025 systems over a 2,500-step
sequence (the resident-block function is replaced), the event that orders a batch's calls, a set_system_state issued while an
integrate is queued -- with stubs of the launchers that walk the device table and touch every byte the kernels would.

  * as a program of its own under AddressSanitizer + UBSan (g++ -O1) and plain (g++ -O1): no failure, no report, the same output;
  * the table the host built for mixed sizes (first-particle indices, dynamic LDS bytes) against numpy, 56 | 57 included.

No GPU; nothing loaded into Python runs under a sanitizer."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "particles_batch_harness.cpp")
COMMON = ["-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")]
_outputs = {}


def _build_and_run(tmp_path_factory, name, flags):
    if name in _outputs:
        return _outputs[name]
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    exe = str(tmp_path_factory.mktemp("particles_batch") / name)
    subprocess.check_call(["g++"] + flags + COMMON + [SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(p.stdout[-8000:])
    assert "FAILED" not in p.stdout, "\n".join(l for l in p.stdout.splitlines() if "FAILED" in l)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-2000:]
    _outputs[name] = p.stdout
    return p.stdout


def _sanitized(tmp_path_factory):
    return _build_and_run(tmp_path_factory, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


def test_batch_life_cycle_refusals_launch_rule_and_ordering(tmp_path_factory):
    san = _sanitized(tmp_path_factory)
    plain = _build_and_run(tmp_path_factory, "plain", ["-O1"])
    assert san == plain
    lines = san.splitlines()
    assert len(lines) == 38 and all(l.endswith(": ok") or l.endswith(" ok") for l in lines[:-1])
    assert lines[-1] == "waits=4 records=5 displays=1 failures=0", lines[-1]
    rule = [l for l in lines if l.startswith("launch rule: ")]
    assert [int(re.match(r"launch rule: (\d+) systems at R = 4: (\d+) rounds", l).group(2)) for l in rule] == [1, 1, 2, 3, 257]


def test_the_hosts_table_matches_numpy_for_mixed_sizes(tmp_path_factory):
    seen = []
    for line in _sanitized(tmp_path_factory).splitlines():
        m = re.match(r"table sizes=([\d,]+) first=([\d,]+) lds=(\d+) n_max=(\d+) total=(\d+) ok$", line)
        if not m:
            continue
        n = np.array(m.group(1).split(","), dtype=np.int64)
        first = np.concatenate([[0], np.cumsum(n)[:-1]])
        pairs = n.max() * (n.max() - 1) // 2 if n.max() <= 56 else 0
        lds = sum(-(-b // 16) * 16 for b in (24 * n.max(), 8 * n.max(), 8 * 201, 8 * 201, 32, 24 * pairs, 4 * pairs))
        assert m.group(2).split(",") == [str(x) for x in first] and int(m.group(3)) == lds, line
        assert int(m.group(4)) == n.max() and int(m.group(5)) == n.sum(), line
        seen.append(int(n.max()))
    assert 56 in seen and 57 in seen and 256 in seen and len(seen) == 5
