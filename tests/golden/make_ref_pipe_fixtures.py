#!/usr/bin/env python3
"""Records what the compiled reference does in pipe mode, for the cases of tests/test_ref_pipe.py's REF_PIPE_CASES: tests/golden/ref_pipe.npz.

  make -C oracle ref && python tests/golden/make_ref_pipe_fixtures.py

For every case the binary (oracle/_ref/ctucopy4_ref: the reference's sources, unchanged, against the FFTW stand-in) runs twice on the same
input bytes, under `timeout` and a file-size limit: once as `... -online_in -online_out` with the bytes on stdin, once as `... -i in -o out`.
Stored per case <c>:
  <c>__input         [bytes, CRC32] of the input, which the test regenerates
  <c>__pipe_status   exit status of the pipe run           <c>__stdout   what it wrote to stdout, as uint8
  <c>__file_status   exit status of the file run           <c>__file     the bytes of the file it wrote, as uint8
  <c>__pipe_vad, <c>__file_vad   (cases with the VAD module) the bytes of -vad_out's file of either run
Neither this script nor the binary is run by a test: the tests read the .npz.
"""
import os
import resource
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.test_ref_pipe import REF_PIPE_CASES  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "ctucopy4_ref")
TIME_LIMIT = 300
FILE_LIMIT = 64 << 20


def run_bin(args, cwd, data=None):
    r = subprocess.run(["timeout", "-k", "5", str(TIME_LIMIT), BIN] + list(args), cwd=cwd, input=data, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                       preexec_fn=lambda: resource.setrlimit(resource.RLIMIT_FSIZE, (FILE_LIMIT, FILE_LIMIT)))
    return (r.returncode if r.returncode >= 0 else 128 - r.returncode), r.stdout


def main():
    if not os.path.exists(BIN):
        raise SystemExit(BIN + " is missing: make -C oracle ref")
    z = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (cfg, make_input, htk, vad) in sorted(REF_PIPE_CASES.items()):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            data = make_input()
            with open(os.path.join(d, "in"), "wb") as f:
                f.write(data)
            z[name + "__input"] = np.array([len(data), zlib.crc32(data)], dtype=np.int64)
            status, out = run_bin(list(cfg) + ["-online_in", "-online_out"] + (["-vad_out", "vad_pipe"] if vad else []), d, data)
            z[name + "__pipe_status"] = np.array(status, dtype=np.int64)
            z[name + "__stdout"] = np.frombuffer(out, dtype=np.uint8)
            status, _ = run_bin(list(cfg) + ["-i", "in", "-o", "out"] + (["-vad_out", "vad_file"] if vad else []), d)
            z[name + "__file_status"] = np.array(status, dtype=np.int64)
            path = os.path.join(d, "out")
            z[name + "__file"] = np.fromfile(path, dtype=np.uint8) if os.path.exists(path) else np.zeros(0, np.uint8)
            if vad:
                for run in ("pipe", "file"):
                    vp = os.path.join(d, "vad_" + run)
                    z[f"{name}__{run}_vad"] = np.fromfile(vp, dtype=np.uint8) if os.path.exists(vp) else np.zeros(0, np.uint8)
            print(name, "pipe", int(z[name + "__pipe_status"]), len(out), "bytes; file", status, z[name + "__file"].size, "bytes;",
                  "stdout == payload" if out == z[name + "__file"].tobytes()[(12 if htk else 0):] else "stdout differs from the payload")
    out_path = os.path.join(HERE, "ref_pipe.npz")
    np.savez_compressed(out_path, **z)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
