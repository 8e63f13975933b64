"""The tick's host twin (tools/host_tick.cpp) as a stand-alone program under sanitizers: every other test runs it inside python, where no
sanitizer sees it."""
import os
import subprocess

import numpy as np

from oracle import oracle_py as orc
from quadruped_drake_amd import workloads

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_twin_stand_alone_under_sanitizers(tmp_path):
    """tools/host_tick_check.cpp and tools/host_tick.cpp compiled into ONE executable, twice, and run as child processes (no shared object in this
    process, no preloaded runtime).  Address + undefined: host_hex_batch for the four laws and a torque box, a warm host_hex_rollout of 2 robots x 5
    ticks, then the first batch again -- and once more after a vdot sink was set and cleared -- with the bits of the first time: a call remembers
    nothing of the calls before it.  Thread: host_tick_bench alone (no fibres), 4 threads x 6 passes over 16 instances: the passes before the last
    write thread-private scratch, so a thread that is a pass behind shares no output element with one that is ahead."""
    data = str(tmp_path / "inputs.bin")
    with open(data, "wb") as f:
        f.write(np.ascontiguousarray(orc.load_model_json("mini_cheetah")["flat"], dtype=np.float64).tobytes())
        for cfg in (2, 3):
            b = workloads.make_batch(cfg, n=8)
            assert b["model"] == "mini_cheetah"
            for a in (b["q"], b["v"], b["targets"]):
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(b["mask"], dtype=np.uint8).tobytes())
    # the compiler of test_no_unwritten_storage_feeds_the_arithmetic where there is one: it instruments this file in half of g++'s time and links
    # the sanitizers' runtimes into the executable
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    builds = []
    for mode, san in (("hex", "address,undefined"), ("bench", "thread")):      # the two compiles side by side
        exe = str(tmp_path / ("host_tick_check_" + mode))
        builds.append((mode, exe, subprocess.Popen([clang if os.path.exists(clang) else "g++", "-O2", "-std=c++20", "-pthread", "-ffp-contract=off", "-fsanitize=" + san, "-o", exe,
                                                    os.path.join(_ROOT, "tools", "host_tick_check.cpp"), os.path.join(_ROOT, "tools", "host_tick.cpp")])))
    for mode, exe, proc in builds:
        assert proc.wait() == 0, mode
    runs = [(mode, subprocess.Popen([exe, mode, data], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for mode, exe, _ in builds]
    for mode, proc in runs:
        out = proc.communicate()[0]
        assert proc.returncode == 0, (mode, out[-4000:])
        # (ASan's one-line notice that it does not fully support makecontext is no report and does not carry its full name)
        assert "AddressSanitizer" not in out and "runtime error" not in out and "ThreadSanitizer: data race" not in out, (mode, out[-4000:])
