"""The signal descriptors of the push planner (ctucopy_amd/csrc/stream_plan.h: a set with signal state - where every stream's samples
go, which frames of the push they are made of, the capacity check, the finish twin), without a GPU and without the engine library.

tests/host/stream_signal_plan_check.cc is a program of its own: it includes the one header, carries a brute-force restatement, and is
built and run under Address + UndefinedBehavior sanitizers, as tests/test_stream_plan_cpu.py builds its program.  Exit status 0, a
final ok line and a silent stderr are the result.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error")


def test_stream_signal_plan_check_under_sanitizers(tmp_path):
    exe = tmp_path / "stream_signal_plan_check"
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "ctucopy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "stream_signal_plan_check.cc"), "-o", str(exe)], check=True)
    cp = subprocess.run([str(exe)], capture_output=True, text=True)
    print(cp.stdout, cp.stderr)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout.strip().splitlines()[-1].startswith("stream_signal_plan_check ok"), cp.stdout
    assert not any(r in cp.stderr for r in REPORTS), cp.stderr
    assert cp.stderr.strip() == "", cp.stderr
