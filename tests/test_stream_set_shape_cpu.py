"""What a stream set is (ctucopy_amd/csrc/stream_set_shape.h: the kinds of state, halo, strides, the size of every per-set buffer, the
arithmetic of the ctu_streams_*_step calls), without a GPU and without the engine library.

tests/host/stream_set_shape_check.cc is a program of its own: it includes the one header, builds its designs with opts.cc and design.cc,
carries a table of shapes written down by hand from ctu_streams_create_ex as it stood before the unit existed, and is built and run
under Address + UndefinedBehavior sanitizers.  Exit status 0, a final ok line and a silent stderr are the result.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error")


def test_stream_set_shape_check_under_sanitizers(tmp_path):
    exe = tmp_path / "stream_set_shape_check"
    csrc = os.path.join(ROOT, "ctucopy_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", csrc, os.path.join(ROOT, "tests", "host", "stream_set_shape_check.cc"),
                    os.path.join(csrc, "opts.cc"), os.path.join(csrc, "design.cc"), "-o", str(exe)], check=True)
    cp = subprocess.run([str(exe)], capture_output=True, text=True)
    print(cp.stdout, cp.stderr)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout.strip().splitlines()[-1].startswith("stream_set_shape_check ok"), cp.stdout
    assert not any(r in cp.stderr for r in REPORTS), cp.stderr
    assert cp.stderr.strip() == "", cp.stderr
