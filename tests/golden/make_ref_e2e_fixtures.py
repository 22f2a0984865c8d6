#!/usr/bin/env python3
"""Records what the compiled reference writes, end to end, for the cases of tests/util.py's REF_E2E_CASES: tests/golden/ref_e2e.npz.

  make -C oracle ref && python tests/golden/make_ref_e2e_fixtures.py            # REF_E2E_CASES -> ref_e2e.npz
  make -C oracle ref && python tests/golden/make_ref_e2e_fixtures.py opts       # REF_E2E_OPT_CASES + ref_e2e_file_cases() -> ref_e2e_opts.npz
  make -C oracle ref && python tests/golden/make_ref_e2e_fixtures.py silence    # REF_E2E_SILENCE_CASES -> ref_e2e_silence.npz

oracle/Makefile's `ref` target compiles the sources of a reference tree (REF=<path>), unchanged and at -O0, against the FFTW stand-in
(oracle/fftw_standin/fftw3.h, oracle/fftw_standin.cc) into oracle/_ref/ctucopy4_ref.  For every case this script writes the input
set as raw files into a temporary directory, builds the list file ("<in> <out>", or "<in> <out> <spk> <vadout>" with any -vad_* mode)
and runs the binary once over the whole list (`... -S list`), under `timeout` and a file-size limit.  Stored per case <c> and file <i>:
  <c>__status                  exit status of the run (0; 139 / 134 / 124 for a case the reference cannot run: nothing else is stored then)
  <c>__<i>__input              [samples, CRC32 of the little-endian int16 bytes] of the input, which tests/util.py regenerates
  <c>__<i>__rows, __header     float32 rows of the HTK file and its [nSamples, sampPeriod, sampSize, parmKind]
  <c>__<i>__vad                the bytes of the VAD file ('0' / '1')
  <c>__<i>__pcm                int16 samples of -format_out raw
  <c>__file__<name>            (file cases) the bytes of output file <name> as uint8; <c>__input = CRC32 of every input file's bytes, in name order
Conditions asserted here and again by tests/test_oracle_ref_e2e.py: every row of the first seven edge inputs is finite; on zeros_mid
the non-finite rows are exactly the frames wholly inside the zero block, at most a quarter of the file's rows.  On the silence table
(tests/util.py's check_silence_conditions, asserted again by tests/test_oracle_ref_e2e_silence.py): the recorded non-finite rows of the first
file, ten finite rows and more on either side of them, a finite second file.
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
from tests.util import (EDGE_INPUTS, REF_E2E_CASES, REF_E2E_OPT_CASES, REF_E2E_SILENCE_CASES, SILENCE_DIES, check_silence_conditions,  # noqa: E402
                        ref_e2e_file_cases, ref_e2e_inputs, zeros_mid_parts)

BIN = os.path.join(ROOT, "oracle", "_ref", "ctucopy4_ref")
TABLES = {"base": (REF_E2E_CASES, False, "ref_e2e.npz"), "opts": (REF_E2E_OPT_CASES, True, "ref_e2e_opts.npz"),   # cases, file cases too, output
          "silence": (REF_E2E_SILENCE_CASES, False, "ref_e2e_silence.npz")}
TIME_LIMIT = 300            # seconds per case; the direct transforms make a 2048-point frame a few milliseconds
FILE_LIMIT = 64 << 20       # bytes: an -O2 build's endless VAD flush wrote gigabytes


def input_id(u):
    return np.array([u.size, zlib.crc32(u.astype("<i2").tobytes())], dtype=np.int64)


def read_htk(path, big_endian=False):
    """Byte order as -endian_out says: the file's length cannot tell (a 0-frame file fits both orders)."""
    raw = open(path, "rb").read()
    e = ">" if big_endian else "<"
    n, period = np.frombuffer(raw[:8], e + "u4")
    size, kind = np.frombuffer(raw[8:12], e + "u2")
    if 12 + int(n) * int(size) != len(raw) or size % 4:
        raise SystemExit(f"{path}: not an HTK file ({len(raw)} bytes)")
    rows = np.frombuffer(raw[12:], e + "f4").astype(np.float32).reshape(int(n), size // 4) if size else np.zeros((0, 0), np.float32)
    return rows, np.array([n, period, size, kind], dtype=np.int64)


def run_bin(cfg, d):
    r = subprocess.run(["timeout", "-k", "5", str(TIME_LIMIT), BIN] + list(cfg) + ["-S", "list"], cwd=d, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, preexec_fn=lambda: resource.setrlimit(resource.RLIMIT_FSIZE, (FILE_LIMIT, FILE_LIMIT)))
    return r.returncode if r.returncode >= 0 else 128 - r.returncode


def run_file_case(name, case, tmp):
    cfg, files, list_text, outputs = case
    d = os.path.join(tmp, name)
    os.makedirs(d)
    for fn, data in files.items():
        with open(os.path.join(d, fn), "wb") as f:
            f.write(data)
    with open(os.path.join(d, "list"), "w") as f:
        f.write(list_text)
    status = run_bin(cfg, d)
    z = {f"{name}__status": np.array(status, dtype=np.int64)}
    if status:
        return z
    z[f"{name}__input"] = np.array([zlib.crc32(files[fn]) for fn in sorted(files)], dtype=np.int64)
    for fn in outputs:
        z[f"{name}__file__{fn}"] = np.fromfile(os.path.join(d, fn), dtype=np.uint8)
    return z


def zero_block_frames(cfg, n, rows):
    """Frames of zeros_mid(n) that lie wholly inside the zero block (with pre-emphasis: the sample in front of the frame too)."""
    opt = {k: v for k, v in zip(cfg[:-1], cfg[1:]) if k.startswith("-")}
    fs = int(opt["-fs"])
    window, shift = int(float(opt.get("-w", 25)) * fs / 1000), int(float(opt.get("-s", 10)) * fs / 1000)
    a, z, _ = zeros_mid_parts(n)
    hist = 1 if float(opt.get("-preem", 0)) > 0 else 0
    starts = np.arange(rows) * shift
    return (starts - hist >= a) & (starts + window <= a + z)


def run_case(name, cfg, inputs, tmp):
    d = os.path.join(tmp, name)
    os.makedirs(d)
    four = any(a.startswith("-vad_") for a in cfg)
    signal = cfg[cfg.index("-format_out") + 1] == "raw"
    lines = []
    for i, u in enumerate(inputs):
        u.astype("<i2").tofile(os.path.join(d, f"in{i}.raw"))
        lines.append(f"{d}/in{i}.raw {d}/out{i}" + (f" spk {d}/vad{i}" if four else ""))
    with open(os.path.join(d, "list"), "w") as f:
        f.write("\n".join(lines) + "\n")
    status = run_bin(cfg, d)
    big = "-endian_out" in cfg and cfg[len(cfg) - 1 - cfg[::-1].index("-endian_out") + 1] == "big"
    z = {f"{name}__status": np.array(status, dtype=np.int64)}
    if status:
        return z
    for i, u in enumerate(inputs):
        z[f"{name}__{i}__input"] = input_id(u)
        if signal:
            z[f"{name}__{i}__pcm"] = np.fromfile(os.path.join(d, f"out{i}"), dtype="<i2").astype(np.int16)
        else:
            z[f"{name}__{i}__rows"], z[f"{name}__{i}__header"] = read_htk(os.path.join(d, f"out{i}"), big)
        if four:
            z[f"{name}__{i}__vad"] = np.fromfile(os.path.join(d, f"vad{i}"), dtype=np.uint8) if os.path.exists(os.path.join(d, f"vad{i}")) else np.zeros(0, np.uint8)
    return z


def check_edge_conditions(name, cfg, inputs, z):
    if cfg[cfg.index("-format_out") + 1] == "raw":
        return
    for i, g in enumerate(EDGE_INPUTS):
        rows = z[f"{name}__{i}__rows"]
        bad = ~np.isfinite(rows).all(axis=1)
        if g != "zeros_mid":
            assert not bad.any(), (name, g, int(bad.sum()))
        else:
            want = zero_block_frames(cfg, inputs[i].size, rows.shape[0])
            assert np.array_equal(bad, want), (name, np.flatnonzero(bad), np.flatnonzero(want))
            assert 0 < bad.sum() <= rows.shape[0] / 4, (name, int(bad.sum()), rows.shape[0])


def main():
    if not os.path.exists(BIN):
        raise SystemExit(f"{BIN} is missing: build it first (make -C oracle ref REF=<reference tree>)")
    which = sys.argv[1] if len(sys.argv) > 1 else "base"
    if which not in TABLES:
        raise SystemExit(f"usage: {sys.argv[0]} [{' | '.join(TABLES)}]")
    cases, with_files, out_name = TABLES[which]
    out_path = os.path.join(HERE, out_name)
    z, sets = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (cfg, inp) in cases.items():
            inputs = sets.setdefault(inp, ref_e2e_inputs(inp))
            got = run_case(name, cfg, inputs, tmp)
            status = int(got[f"{name}__status"])
            print(f"{name}: status {status}" + ("" if status else f", {sum(v.nbytes for v in got.values())} bytes"))
            if not status and inp.startswith("edge"):
                check_edge_conditions(name, cfg, inputs, got)
            if inp.startswith("sil"):
                assert status == SILENCE_DIES.get(name, 0), (name, status)
                if not status and f"{name}__0__rows" in got:
                    check_silence_conditions(name, cfg, got[f"{name}__0__rows"], got[f"{name}__1__rows"])
            z.update(got)
        for name, case in (ref_e2e_file_cases() if with_files else {}).items():
            got = run_file_case(name, case, tmp)
            status = int(got[f"{name}__status"])
            print(f"{name}: status {status}" + ("" if status else f", {sum(v.nbytes for v in got.values())} bytes"))
            z.update(got)
    np.savez_compressed(out_path, **z)
    print(out_path, os.path.getsize(out_path))


if __name__ == "__main__":
    main()
