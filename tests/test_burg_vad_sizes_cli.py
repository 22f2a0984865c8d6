"""bin/ctucopy with the Burg-cepstral VAD on 44.1 kHz audio (1103 samples, 2048 points): a list is walked like the reference walks
it - the majority filter's ring index runs on from file to file (src/vad/vad.h:110-121) - in one engine or spread over two."""
import struct
import subprocess

import numpy as np
import pytest

from ctucopy_amd import build as cbuild
from oracle.oracle import Oracle
from tests.util import synth_utt

CFG = ("-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97 -vad burg -vad_out_mode vad -vad_cri_mode cepdist "
       "-vad_cepdist_mode lpc -vad_thr_mode adapt").split()


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_cli()


@pytest.mark.gpu
def test_burg_vad_list_at_44k_through_the_cli_is_the_reference_list(tmp_path):
    utts, lines = [], []
    for i, n in enumerate((40000, 47111, 54222)):
        u = synth_utt(130 + i, n)
        u.astype("<i2").tofile(tmp_path / f"u{i}.raw")
        utts.append(u)
        lines.append(f"{tmp_path / f'u{i}.raw'} {tmp_path / f'u{i}.htk'} spk {tmp_path / f'u{i}.vad'}")
    (tmp_path / "list").write_text("\n".join(lines) + "\n")
    ref = Oracle(CFG).process_list(utts, want_vad=True)
    assert [rv.size for _, rv in ref] == [89, 105, 121]
    assert all(0 < int((rv == ord("1")).sum()) < rv.size for _, rv in ref)   # mixed decisions in every file
    images = []
    for extra in ([], ["--gpus", "2", "--gpu-map", "0,0"]):
        r = subprocess.run([cbuild.CLI] + CFG + ["-S", str(tmp_path / "list")] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for i, (rows, rv) in enumerate(ref):
            raw = (tmp_path / f"u{i}.htk").read_bytes()
            n = struct.unpack("<I", raw[:4])[0]
            assert n == rows.shape[0] and (tmp_path / f"u{i}.vad").read_bytes() == bytes(rv), (extra, i)
            got = np.frombuffer(raw[12:], dtype="<f4").reshape(n, -1)
            assert np.array_equal(~got.any(axis=1), ~rows.any(axis=1))
            assert np.all(np.abs(got - rows) <= 1e-3 * np.maximum(np.abs(rows), 1.0)), (extra, i)
        images.append([(tmp_path / f"u{i}.htk").read_bytes() + (tmp_path / f"u{i}.vad").read_bytes() for i in range(3)])
    assert images[0] == images[1]   # two engines write the same bytes
