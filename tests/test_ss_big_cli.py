"""bin/ctucopy with -nr_mode fwss -vad burg on 44.1 kHz audio (1103 samples, 2048 points: bigss_kernel.h): the files of a list are
chained through the noise seed (src/nr/nr.cc:212-221), so the CLI runs them on one GPU in list order - in one batch or in several."""
import struct
import subprocess

import numpy as np
import pytest

from ctucopy_amd import build as cbuild
from tests.test_ss_big import the_list

CFG = "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97 -nr_mode fwss -vad burg".split()
SIG = "-fs 44100 -format_in raw -format_out raw -preset exten -nr_mode fwss -vad burg".split()


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_cli()


def _write_list(tmp_path, utts, ext):
    lines = []
    for i, u in enumerate(utts):
        u.astype("<i2").tofile(tmp_path / f"u{i}.raw")
        lines.append(f"{tmp_path / f'u{i}.raw'} {tmp_path / f'u{i}.{ext}'}")
    (tmp_path / "list").write_text("\n".join(lines) + "\n")


@pytest.mark.gpu
def test_fwss_list_at_44k_through_the_cli_is_the_engines_list(tmp_path):
    from ctucopy_amd import Engine
    utts = the_list(CFG) * 3   # three times over: 666 099 samples, which --batch-mib 1 (524 288 samples a batch) cuts into two batches
    _write_list(tmp_path, utts, "htk")
    eng = Engine(CFG)
    rows = eng.extract(utts)
    assert [r.shape[0] for r in rows] == [89, 105, 121, 111, 0, 66] * 3
    assert not np.array_equal(rows[0], rows[6])   # the same samples behind another file: another seed
    images = []
    for extra in ([], ["--batch-mib", "1"], ["--gpus", "2", "--gpu-map", "0,0"]):   # two engines asked for: one is used, files in list order
        r = subprocess.run([cbuild.CLI] + CFG + ["-S", str(tmp_path / "list")] + extra, capture_output=True, text=True)
        assert r.returncode == 0, (extra, r.stderr)
        for i, want in enumerate(rows):
            raw = (tmp_path / f"u{i}.htk").read_bytes()
            assert struct.unpack("<IIHH", raw[:12]) == (want.shape[0], 100000, 52, 8198), (extra, i)
            got = np.frombuffer(raw[12:], dtype="<f4").reshape(want.shape[0], 13)
            assert np.array_equal(got, want), (extra, i)
        images.append([(tmp_path / f"u{i}.htk").read_bytes() for i in range(len(utts))])
    assert images[0] == images[1] == images[2]


@pytest.mark.gpu
def test_fwss_speech_output_at_44k_through_the_cli(tmp_path):
    from ctucopy_amd import Engine
    utts = the_list(SIG)[:3]
    _write_list(tmp_path, utts, "out")
    want = Engine(SIG).enhance(utts)
    r = subprocess.run([cbuild.CLI] + SIG + ["-S", str(tmp_path / "list")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for i, w in enumerate(want):
        got = np.frombuffer((tmp_path / f"u{i}.out").read_bytes(), dtype="<i2")
        assert got.size == [39535, 46595, 53655][i] and np.array_equal(got, w), i
