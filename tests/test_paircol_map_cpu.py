"""The index maps of the pair-column second stage (ctucopy_amd/csrc/paircol_map.h), without a GPU.

tests/host/paircol_map_check.cc includes the header - whose static_asserts thereby compile on the host - and enumerates a whole step:
where stage 1's stores land, what stage 2's read pairs return, the untangle's partner (column, register) of all 16 x 16 elements of a
frame with lane p = 0's two self-mirrored columns, the twiddle record per half, bins 0..256 each produced once, the fit and offset
conditions, and the transposed reads' LDS cycles under the 32-lane / 32-bank host model against the layout they replace.  Built with
the host compiler under Address+UB sanitizers as a program of its own and run directly: nothing is loaded into python or preloaded."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_paircol_maps_by_enumeration(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "paircol_map_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ctucopy_amd", "csrc"), os.path.join(ROOT, "tests", "host", "paircol_map_check.cc"),
                    "-o", str(exe)], check=True)
    cp = subprocess.run([str(exe)], capture_output=True, text=True)
    assert cp.returncode == 0, cp.stderr[-4000:]
    assert cp.stderr == "", cp.stderr[-4000:]
    assert cp.stdout.startswith("paircol_map_check ok: reads 64 cycles"), cp.stdout
