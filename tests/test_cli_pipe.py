"""Pipe mode of bin/ctucopy on a device: -online_in / -online_out against the tool's own file mode on the same bytes.

The yardstick is what `bin/ctucopy -i in -o out` writes.  A pipe pushes its samples in pieces that end a multiple of eight frames into the
file (ctucopy_amd/host/pipe.h: pipe_take), the condition under which include/ctu_engine.h promises the rows, decisions and samples of the
offline run bit for bit - so the comparison is byte for byte, with one exception the header names: C5's trapdct below the fp32 kernel's
sizes, where the offline run splits its operands into fp16 terms and the stream contracts in fp32; there the bound is the one
tests/test_streams_trap.py:123 applies to the same pair (_assert_rows of tests/test_gpu_parity.py).  Pipe mode adds no arithmetic.

Every run is a fresh child process under a time limit; a file-mode result is computed once and shared by the cases that compare with it.
"""
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

from ctucopy_amd import build as cbuild
from tests.test_ref_pipe import REF_PIPE_CASES, ref_pipe
from tests.util import C1, C2, C4, C5, M44, SIG_EXTEN, g711_codes, sig, wave_image

pytestmark = pytest.mark.gpu
CLI = cbuild.CLI
LIMIT = 120


def _le(x):
    return np.asarray(x, dtype="<i2").tobytes()


CS3 = _le(sig("CS3")[:32000])          # 2 s at 16 kHz
CS0 = _le(sig("CS0")[:32000])
CS3_8K = _le(sig("CS3")[:32000:2])     # 2 s at 8 kHz
NOISE = _le(np.random.default_rng(20).integers(-3000, 3000, 16000))
ALAW = "-fs 8000 -format_in alaw -format_out htk -preset mfcc".split()
MULAW = "-fs 8000 -format_in mulaw -format_out htk -preset mfcc".split()
SIG44 = "-fs 44100 -format_in raw -format_out raw -preset exten".split()
DELTA = C2 + ["-fea_delta", "d_a", "-fea_Z_exp", "500"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_cli()


def _with(cfg, key, value):
    out = list(cfg)
    out[out.index(key) + 1] = value
    return out


def run(args, data=None):
    return subprocess.run([CLI] + [str(a) for a in args], input=data, capture_output=True, timeout=LIMIT)


_offline = {}


@pytest.fixture(scope="module")
def offline(tmp_path_factory):
    """(status, stderr, output file's bytes or None, VAD file's bytes or None) of `bin/ctucopy cfg -i in -o out [-vad_out v]`, once per key."""
    def get(key, cfg, data, vad=False):
        if key not in _offline:
            d = tmp_path_factory.mktemp("offline")
            (d / "in").write_bytes(data)
            r = run(list(cfg) + ["-i", d / "in", "-o", d / "out"] + (["-vad_out", d / "v"] if vad else []))
            _offline[key] = (r.returncode, r.stderr, (d / "out").read_bytes() if (d / "out").exists() else None,
                             (d / "v").read_bytes() if (d / "v").exists() else None)
        return _offline[key]
    return get


def pipe(cfg, data, *extra):
    return run(list(cfg) + ["-online_in", "-online_out"] + list(extra), data)


def _rows(payload, width=13):
    return np.frombuffer(payload, "<f4").reshape(-1, width)


# ---- 1: stdin to stdout, whatever the reads
@pytest.mark.parametrize("read", [None, 4096, 7])
def test_c1_stdin_to_stdout_equals_the_files_payload_for_every_read_size(offline, read):
    status, _, img, _ = offline("c1", C1, CS3)
    assert status == 0 and len(img) == 12 + 198 * 52
    r = pipe(C1, CS3, *(["--pipe-read-bytes", read] if read else []))
    assert r.returncode == 0, r.stderr
    assert r.stdout == img[12:]
    assert r.stderr == b""


def test_c1_with_the_vad_module_against_the_reference_pipe(tmp_path):
    """The reference dies in single-file mode without a VAD module (tests/test_ref_pipe.py), so its pipe's rows exist for C1 with the
    energy detector beside it: the same rows within tests/test_cli.py's _close, the same decisions."""
    from tests.test_cli import _close
    cfg, make_input, _, _ = REF_PIPE_CASES["c1_vad"]
    z = ref_pipe()
    r = pipe(cfg, make_input(), "-vad_out", tmp_path / "v")
    assert r.returncode == 0, r.stderr
    ref = _rows(z["c1_vad__stdout"].tobytes())
    got = _rows(r.stdout)
    assert got.shape == ref.shape == (98, 13)
    print("largest |got - ref| / max(|ref|, 1):", float((np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)).max()))
    assert _close(got, ref)
    assert (tmp_path / "v").read_bytes() == z["c1_vad__pipe_vad"].tobytes()


# ---- 2: the mixed combinations, either byte order
@pytest.mark.parametrize("endian", ["little", "big"])
def test_c1_stdin_to_a_file_and_a_file_to_stdout(offline, tmp_path, endian):
    cfg = C1 + ["-endian_out", endian]
    status, _, img, _ = offline("c1-" + endian, cfg, CS3)
    assert status == 0 and struct.unpack("<I" if endian == "little" else ">I", img[:4])[0] == 198
    r = run(cfg + ["-online_in", "-o", tmp_path / "f"], CS3)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert (tmp_path / "f").read_bytes() == img
    (tmp_path / "in").write_bytes(CS3)
    r = run(cfg + ["-i", tmp_path / "in", "-online_out"])
    assert r.returncode == 0, r.stderr
    assert r.stdout == img[12:]


# ---- 3 .. 8: the kinds of state and the inputs, pipe against file
# name -> (command line, input, extra host flags, width of a row or 0 for samples)
EQUAL_CASES = {
    "row state: d_a + CMS": (DELTA, CS3, [], 39),
    "subtraction state: fwss": (C2 + ["-nr_mode", "fwss", "-vad", "burg"], CS3, [], 13),
    "large state: exten features at 44.1 kHz": (M44 + ["-nr_mode", "exten"], CS3, [], 13),
    "signal state: exten at 16 kHz": (SIG_EXTEN, CS3, [], 0),
    "signal + large state: exten at 44.1 kHz": (SIG44, CS3, [], 0),
    "a-law": (ALAW, g711_codes(8000).tobytes(), ["--pipe-read-bytes", 4097], 13),
    "mu-law": (MULAW, g711_codes(8000).tobytes(), ["--pipe-read-bytes", 4097], 13),
    "wave in reads of 5 bytes": (_with(C1, "-format_in", "wave"), wave_image(np.frombuffer(NOISE, "<i2")), ["--pipe-read-bytes", 5], 13),
    "-endian_in big": (_with(C1, "-endian_in", "big"), NOISE, ["--pipe-read-bytes", 4097], 13),
}


@pytest.mark.parametrize("name", sorted(EQUAL_CASES))
def test_pipe_equals_file_mode_byte_for_byte(offline, name):
    cfg, data, extra, width = EQUAL_CASES[name]
    status, err, img, _ = offline(name, cfg, data)
    assert status == 0 and img, err
    r = pipe(cfg, data, *extra)
    assert r.returncode == 0, r.stderr
    want = img[12:] if width else img
    assert len(r.stdout) == len(want) and len(want) > 0
    if width:
        assert struct.unpack("<IIH", img[:10])[2] == 4 * width and np.isfinite(_rows(want, width)).all()
    assert r.stdout == want


def test_wave_output_to_a_file_equals_file_mode(offline, tmp_path):
    cfg = _with(SIG_EXTEN, "-format_out", "wave")
    status, err, img, _ = offline("wave out", cfg, CS3)
    assert status == 0 and img[:4] == b"RIFF", err
    r = run(cfg + ["-online_in", "-o", tmp_path / "f.wav", "--pipe-read-bytes", 4096], CS3)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert (tmp_path / "f.wav").read_bytes() == img


def test_a_chain_on_too_few_frames_fails_as_file_mode_does(offline):
    # d_a: windows of 2 and 2, wmax + 1 = 3 frames
    data = CS3[:2 * (400 + 2 * 160)]
    status, err, img, _ = offline("delta short", DELTA, data)
    assert status == 255 and b"fewer than window+2 frames" in err and img is None
    r = pipe(DELTA, data, "--pipe-read-bytes", 512)
    assert (r.returncode, r.stderr) == (status, err)
    assert r.stdout == b""


# ---- 4: the VAD module
@pytest.mark.parametrize("mode", ["none", "drop"])
def test_c4_rows_and_decisions_equal_file_mode(offline, tmp_path, mode):
    cfg = C4 + ["-vad_apply_mode", mode]
    status, err, img, vad = offline("c4-" + mode, cfg, CS3_8K, vad=True)
    assert status == 0 and vad and len(vad) == 198 and set(vad) <= set(b"01"), err
    assert 0 < vad.count(b"1") < len(vad)
    assert len(img) == 12 + 198 * 52 if mode == "none" else 12 < len(img) < 12 + 198 * 52   # drop: fewer rows than frames
    r = pipe(cfg, CS3_8K, "-vad_out", tmp_path / "v", "--pipe-read-bytes", 4096)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "v").read_bytes() == vad
    assert r.stdout == img[12:]


def test_a_file_the_majority_filter_never_releases_writes_nothing(offline, tmp_path):
    cfg = C4 + ["-vad_filter_order", "7"]
    data = CS3_8K[:2 * (200 + 2 * 80)]   # 3 frames of 25 / 10 ms at 8 kHz: no more than (7 - 1) / 2
    status, err, img, vad = offline("c4 short", cfg, data, vad=True)
    assert status == 0 and vad == b"" and len(img) == 12, err
    r = pipe(cfg, data, "-vad_out", tmp_path / "v")
    assert (r.returncode, r.stderr) == (0, err)
    assert r.stdout == b"" and (tmp_path / "v").read_bytes() == b""


# ---- 7: trapdct
def test_c5_trapdct_within_the_stream_tests_bound(offline):
    from tests.test_gpu_parity import _assert_rows
    status, err, img, _ = offline("c5", C5, CS0)
    assert status == 0, err
    r = pipe(C5, CS0)
    assert r.returncode == 0, r.stderr
    off, got = _rows(img[12:], 23 * 16), _rows(r.stdout, 23 * 16)
    assert got.shape == off.shape == (198, 23 * 16) and np.isfinite(got).all()
    print("C5 pipe (fp32 MFMA) vs file mode (fp16 split), largest |difference| / max(|offline|, 1):",
          float((np.abs(got - off) / np.maximum(np.abs(off), 1.0)).max()))
    _assert_rows(got, off, C5)   # the bound of tests/test_streams_trap.py:123 on the same pair of kernels


# ---- 9: inputs that hold no frame
@pytest.mark.parametrize("nbytes", [0, 1, 2 * (400 - 160 - 1)])
def test_inputs_shorter_than_a_frame_fail_as_file_mode_does(offline, nbytes):
    data = CS3[:nbytes]
    status, err, img, _ = offline("short-%d" % nbytes, C1, data)
    assert status == 255 and err == b"IO: Signal shorter than one frame!\n" and img is None
    r = pipe(C1, data)
    assert (r.returncode, r.stderr, r.stdout) == (status, err, b"")


def test_speech_output_of_an_input_without_a_frame_equals_file_mode(offline):
    data = CS3[:2 * 300]   # -preset exten at 16 kHz: 512 / 256 samples; 256 <= 300 < 512 is an input, and no frame
    status, err, img, _ = offline("signal no frame", SIG_EXTEN, data)
    print("file mode:", status, err, None if img is None else len(img))
    r = pipe(SIG_EXTEN, data)
    assert (r.returncode, r.stderr, r.stdout) == (status, err, img or b"")
    assert status == 0 and img == bytes(2 * 256)   # the writer's close() puts out its cache of window - wshift samples, all zero


# ---- 10: a stream, not "read everything, then run"
def test_rows_leave_while_stdin_is_still_open(offline):
    status, _, img, _ = offline("c1", C1, CS3)
    assert status == 0
    first = 2 * (63 * 160 + 400)   # the samples that complete 64 frames
    want = 64 * 52
    child = subprocess.Popen([CLI] + C1 + ["-online_in", "-online_out"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    got = bytearray()

    def reader():
        while len(got) < want:
            piece = os.read(child.stdout.fileno(), want - len(got))
            if not piece:
                return
            got.extend(piece)

    t = threading.Thread(target=reader, daemon=True)
    try:
        child.stdin.write(CS3[:first])
        child.stdin.flush()
        t.start()
        t.join(60)
        if t.is_alive() or len(got) != want:
            child.kill()
            pytest.fail("no rows while stdin was open: %d of %d bytes; stderr: %r" % (len(got), want, child.stderr.read() if not t.is_alive() else b""))
        assert bytes(got) == img[12:12 + want]
        assert child.poll() is None   # it still waits for input
        rest, err = child.communicate(CS3[first:], timeout=LIMIT)
    finally:
        if child.poll() is None:
            child.kill()
            child.wait()
    assert child.returncode == 0, err
    assert bytes(got) + rest == img[12:]
