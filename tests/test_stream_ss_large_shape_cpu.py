"""The stream set that holds subtraction state on large transforms (ctucopy_amd/csrc/stream_set_shape.h with CTU_STREAMS_SS_LARGE_STATE
beside CTU_STREAMS_SS_STATE), without a GPU and without the engine library.

tests/host/stream_ss_large_shape_check.cc is a program of its own: it includes the one header, builds its designs with opts.cc and
design.cc, carries hand-written rows for the new set at 2048 and 4096 points (NIT 8 and 16) and for the engines and sets that do not
fit each other, and is built and run under Address + UndefinedBehavior sanitizers.  Exit status 0, a final ok line and a silent stderr
are the result.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error")


def test_stream_ss_large_shape_check_under_sanitizers(tmp_path):
    exe = tmp_path / "stream_ss_large_shape_check"
    csrc = os.path.join(ROOT, "ctucopy_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", csrc, os.path.join(ROOT, "tests", "host", "stream_ss_large_shape_check.cc"),
                    os.path.join(csrc, "opts.cc"), os.path.join(csrc, "design.cc"), "-o", str(exe)], check=True)
    cp = subprocess.run([str(exe)], capture_output=True, text=True)
    print(cp.stdout, cp.stderr)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout.strip().splitlines()[-1].startswith("stream_ss_large_shape_check ok"), cp.stdout
    assert not any(r in cp.stderr for r in REPORTS), cp.stderr
    assert cp.stderr.strip() == "", cp.stderr
