"""The host side of bin/ctucopy's pipe mode (ctucopy_amd/host/pipe.h, and the serialisation it shares with file mode in files.h), without
a GPU and without the engine library.

tests/host/pipe_check.cc is a program of its own: it includes pipe.h, states the one pure engine function the header calls
(ctu_streams_step) as include/ctu_engine.h documents it, and checks pipe_take against a brute-force count, the byte accumulator and the
WAVE header parser across reads of every awkward size, and the shared row serialiser against write_htk.  It is built and run under
Address + UndefinedBehavior sanitizers.  Exit status 0, a final ok line and a silent stderr are the result.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error")


def test_pipe_check_under_sanitizers(tmp_path):
    exe = tmp_path / "pipe_check"
    csrc = os.path.join(ROOT, "ctucopy_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    "-I", os.path.join(ROOT, "ctucopy_amd", "host"), os.path.join(ROOT, "tests", "host", "pipe_check.cc"),
                    os.path.join(csrc, "opts.cc"), "-o", str(exe)], check=True)
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    cp = subprocess.run([str(exe), str(scratch)], capture_output=True, text=True)
    print(cp.stdout, cp.stderr)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout.strip().splitlines()[-1].startswith("pipe_check ok"), cp.stdout
    assert not any(r in cp.stderr for r in REPORTS), cp.stderr
    assert cp.stderr.strip() == "", cp.stderr
