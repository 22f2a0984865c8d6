"""The `ctucopy` executable's G.711 decoders against the reference's own expander, all 256 codes of both laws.

src/io/amulaw.h is FFTW-free: oracle/Makefile compiles it into oracle/_ref/libref_amulaw.so, and tests/golden/make_ref_fixtures.py
recorded both of its tables in tests/golden/ref_outputs.npz.  The host decoder (ctucopy_amd/host/g711.h) is compiled stand-alone
here; no GPU involved.
"""
import ctypes
import os
import subprocess

import numpy as np

from tests.util import ref_outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_g711_tables_identical_to_reference(tmp_path):
    src = tmp_path / "t.cc"
    src.write_text('#include "g711.h"\nextern "C" void host_table(int alaw, short *o) '
                   '{ for (int v = 0; v < 256; v++) o[v] = g711_to_linear((uint8_t)v, alaw != 0); }\n')
    so = tmp_path / "t.so"
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "ctucopy_amd", "host"), str(src), "-o", str(so)], check=True)
    host, ref = ctypes.CDLL(str(so)), ref_outputs()
    for mode in (0, 1):  # 0 = mu-law, 1 = A-law (src/io/amulaw.h:21)
        a, b = np.zeros(256, dtype=np.int16), ref["amulaw_a" if mode else "amulaw_mu"]
        host.host_table(mode, a.ctypes.data_as(ctypes.c_void_p))
        assert np.array_equal(a, b), mode
        assert len(set(b.tolist())) > 200
