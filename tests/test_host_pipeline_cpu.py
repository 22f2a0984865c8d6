"""The command-line host's plumbing (ctucopy_amd/host/pipeline.h: Chan, parallel_for, per_gpu, PinPool and its owning
handle) and its file readers / writers (files.h), without a GPU and without the engine library.

tests/host/host_check.cc is a program of its own: it includes the two headers, links csrc/opts.cc, and is built and run twice -
under ThreadSanitizer, and under Address + UndefinedBehavior sanitizers.  Exit status 0 and no sanitizer report is the result.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = ("WARNING: ThreadSanitizer", "ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error")


@pytest.mark.parametrize("name,flags", [("thread", ["-O1", "-g", "-fsanitize=thread"]), ("address", ["-fsanitize=address,undefined"])])
def test_host_check_under_sanitizers(tmp_path, name, flags):
    exe = tmp_path / ("host_check_" + name)
    subprocess.run(["g++", "-std=c++17", "-pthread", *flags, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ctucopy_amd", "csrc"),
                    "-I", os.path.join(ROOT, "ctucopy_amd", "host"), os.path.join(ROOT, "tests", "host", "host_check.cc"),
                    os.path.join(ROOT, "ctucopy_amd", "csrc", "opts.cc"), "-o", str(exe)], check=True)
    work = tmp_path / "files"
    work.mkdir()
    cp = subprocess.run([str(exe), str(work)], capture_output=True, text=True)
    print(cp.stdout, cp.stderr)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert "host_check ok" in cp.stdout
    assert not any(r in cp.stderr for r in REPORTS), cp.stderr
    assert cp.stderr.strip() == "", cp.stderr
