"""Offline wire input without a GPU (include/ctu_engine.h: ctu_plan_unpack_wire, ctu_engine_run_wire_host, ctu_engine_run_signal_wire_host;
bin/ctucopy --channels): the symbols, what the command-line host refuses ahead of the engine and of any input, and the host-only parts -
list expansion and target naming, the wire arena of a shard, the covering range of a part, the bound check that precedes a launch, the
pieces the kernel is dealt by - as a program of its own (tests/host/wire_files_check.cc) against brute force, built and run under
Address + UndefinedBehavior sanitizers.  The runs on a device are tests/test_wire_offline.py and tests/test_wire_offline_cli.py."""
import os
import subprocess

import numpy as np
import pytest

from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from tests.util import C1, sig, wave_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = cbuild.CLI
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error")
WIRE_OFFLINE_EXPORTS = ["ctu_plan_unpack_wire", "ctu_engine_run_wire_host", "ctu_engine_run_signal_wire_host"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_cli()


def run(args, data=b""):
    return subprocess.run([CLI] + [str(a) for a in args], input=data, capture_output=True, timeout=120)


def _with(cfg, key, value):
    out = list(cfg)
    out[out.index(key) + 1] = value
    return out


def test_symbols_exported_and_bound():
    L = ceng.load_library()
    for name in WIRE_OFFLINE_EXPORTS:
        assert name in ceng.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    for name in ("unpack_wire_device", "extract_wire", "enhance_wire", "extract_interleaved", "run_wire_host"):
        assert callable(getattr(ceng.Engine, name)), name
    header = open(os.path.join(ROOT, "include", "ctu_engine.h")).read()
    for name in WIRE_OFFLINE_EXPORTS:
        assert f"int {name}(" in header, name


def test_host_parts_under_sanitizers(tmp_path):
    exe = tmp_path / "wire_files_check"
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "ctucopy_amd", "csrc"), "-I", os.path.join(ROOT, "ctucopy_amd", "host"),
                    os.path.join(ROOT, "tests", "host", "wire_files_check.cc"), "-o", str(exe)], check=True)
    cp = subprocess.run([str(exe)], capture_output=True, text=True)
    print(cp.stdout, cp.stderr)
    assert cp.returncode == 0, cp.stdout + cp.stderr
    assert cp.stdout.strip().splitlines()[-1] == "wire_files_check ok", cp.stdout
    assert not any(r in cp.stderr for r in REPORTS), cp.stderr
    assert cp.stderr.strip() == "", cp.stderr


def test_channels_refusals_ahead_of_the_engine(tmp_path):
    """By name, with no device asked for ("no CPU fallback" is what a run that reaches the engine says on a machine without one) and
    nothing written."""
    raw = tmp_path / "in.raw"
    raw.write_bytes(sig("CS3")[:8000].astype("<i2").tobytes())
    out = tmp_path / "out.htk"
    files = C1 + ["-i", raw, "-o", out]
    number = "ENGINE: --channels needs the number of interleaved channels of every input file, 1 or more\n"
    cases = (
        (files + ["--channels", "0"], number),
        (files + ["--channels", "-2"], number),
        (files + ["--channels", "two"], number),
        (files + ["--channels", "2x"], number),
        (files + ["--channels"], number),
        (C1 + ["--channels", "2", "-online_in", "-online_out"],
         "ENGINE: --channels above 1 with -online_in (a pipe is one stream: one set of streams per pipe is not built)\n"),
        (C1 + ["--channels", "2", "-online_in", "-o", out],
         "ENGINE: --channels above 1 with -online_in (a pipe is one stream: one set of streams per pipe is not built)\n"),
        (C1 + ["--channels", "2", "-i", raw, "-online_out"],
         "ENGINE: --channels above 1 with -online_out (a pipe takes one file, --channels writes one per channel)\n"),
        (_with(C1, "-format_in", "htk") + ["-nfeacoefs", "13", "-i", raw, "-o", out, "--channels", "3"],
         "ENGINE: --channels above 1 with -format_in htk (a feature file has rows, not channels)\n"),
    )
    for args, text in cases:
        r = run(args)
        assert r.returncode == 255 and r.stderr.decode() == text, (args, r.stderr)
        assert r.stdout == b"" and not out.exists()


def _stereo_wave(x, channels):
    """The canonical 44-byte header of tests.util.wave_image with its channel fields set for `channels` interleaved channels."""
    img = bytearray(wave_image(np.ascontiguousarray(x).reshape(-1), fs=16000))
    img[22:24] = int(channels).to_bytes(2, "little")
    img[28:32] = (16000 * 2 * channels).to_bytes(4, "little")
    img[32:34] = (2 * channels).to_bytes(2, "little")
    return bytes(img)


def test_wave_channel_count_ahead_of_the_engine(tmp_path):
    x = sig("CS3")[:8000].reshape(-1, 2)
    wav = tmp_path / "stereo.wav"
    wav.write_bytes(_stereo_wave(x, 2))
    out = tmp_path / "out.htk"
    cfg = _with(C1, "-format_in", "wave") + ["-i", wav, "-o", out]
    r = run(cfg)   # without --channels: the reference's words
    assert r.returncode == 255 and r.stderr.decode() == "IN: Input WAVE file is not mono!\n", r.stderr
    r = run(cfg + ["--channels", "3"])
    assert r.returncode == 255 and r.stderr.decode() == "IN: Input WAVE file holds 2 channels, --channels says 3\n", r.stderr
    r = run(cfg + ["--channels", "1"])
    assert r.returncode == 255 and r.stderr.decode() == "IN: Input WAVE file holds 2 channels, --channels says 1\n", r.stderr
    mono = tmp_path / "mono.wav"
    mono.write_bytes(_stereo_wave(x[:, 0], 1))
    r = run(_with(C1, "-format_in", "wave") + ["-i", mono, "-o", out, "--channels", "2"])
    assert r.returncode == 255 and r.stderr.decode() == "IN: Input WAVE file holds 1 channels, --channels says 2\n", r.stderr
    assert not out.exists() and not (tmp_path / "out_1.htk").exists()
