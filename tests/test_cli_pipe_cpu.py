"""Pipe mode of bin/ctucopy (-online_in / -online_out) without a GPU: an accepted configuration gets as far as opening the device, and what
no stream set takes is refused by name ahead of the engine and of the first byte of input (ctu_streams_flags_for, ctucopy_amd/host/main.cc:
pipe_stage).  The runs on a device are tests/test_cli_pipe.py."""
import subprocess

import pytest

from ctucopy_amd import build as cbuild
from tests.util import C1, sig

CLI = cbuild.CLI
PCM = sig("CS3")[:8000].astype("<i2").tobytes()


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_cli()


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")


def run(args, data=PCM):
    return subprocess.run([CLI] + list(args), input=data, capture_output=True, timeout=120)


def _with(cfg, key, value):
    out = list(cfg)
    out[out.index(key) + 1] = value
    return out


def test_pipe_mode_reaches_the_device():
    _no_gpu()
    for args in (C1 + ["-online_in", "-online_out"], C1 + ["-online_in", "-online_out", "--pipe-read-bytes", "7"],
                 C1 + ["--gpus", "2", "-online_in", "-online_out"]):
        r = run(args)
        err = r.stderr.decode()
        assert r.returncode == 255 and "no CPU fallback" in err and "online (pipe) mode is not supported" not in err, err
        assert r.stdout == b""


def test_online_in_to_a_file_and_a_file_to_online_out_reach_the_device(tmp_path):
    _no_gpu()
    raw = tmp_path / "in.raw"
    raw.write_bytes(PCM)
    for args in (C1 + ["-online_in", "-o", str(tmp_path / "out.htk")], C1 + ["-i", str(raw), "-online_out"]):
        r = run(args)
        err = r.stderr.decode()
        assert r.returncode == 255 and "no CPU fallback" in err and "not supported" not in err, err
        assert r.stdout == b"" and not (tmp_path / "out.htk").exists()


def test_what_no_stream_set_takes_is_refused_by_name_ahead_of_the_device():
    lead = "ENGINE: online input: "
    htk_in = _with(C1, "-format_in", "htk")
    cases = (
        (C1 + ["-remove_dc1", "on"], lead + "configuration cannot be streamed: -remove_dc1 (a frame's offset stays subtracted from the samples the later frames share with it)"),
        (htk_in + ["-fea_rawenergy", "on", "-nfeacoefs", "13"], lead + "configuration cannot be streamed: -format_in htk (HTK feature input: there are no samples to stream)"),
        (_with(C1, "-format_out", "ark=" + "x.ark"), lead + "-format_out ark (an archive is written for a list; a pipe writes htk, raw or wave)"),
        (_with(C1, "-format_out", "pfile=" + "x.pf") + ["-o", "x"], lead + "-format_out pfile (an archive is written for a list; a pipe writes htk, raw or wave)"),
        (C1 + ["-stat_cmvn", "stats.txt"], lead + "configuration cannot be streamed: -stat_cmvn / -apply_cmvn (CMVN: statistics over whole lists)"),
        (C1 + ["-nr_mode", "exten", "-nr_when", "afterFB"], None),
        (C1 + ["-vad_out_mode", "vad", "-vad_cri_mode", "cepdist", "-vad_cepdist_mode", "fea", "-vad_out", "v"], None),
        (C1 + ["-nr_mode", "fwss", "-vad", "file=/nonexistent/decisions"], None),
    )
    for args, text in cases:
        online = ["-online_in"] + ([] if "-o" in args else ["-online_out"])
        r = run(args + online)
        err = r.stderr.decode()
        assert r.returncode == 255 and err.startswith(lead) and "no CPU fallback" not in err, (args, err)
        assert text is None or err == text + "\n", (args, err)
        assert r.stdout == b""
    # HTK feature input the engine itself has no path for: its words, behind the same lead
    r = run(htk_in + ["-online_in", "-online_out"])
    assert r.returncode == 255 and r.stderr.decode().startswith(lead) and "HTK feature input" in r.stderr.decode()
    # an input format no reader knows: the reader's words, no device
    r = run(_with(C1, "-format_in", "flac") + ["-online_in", "-online_out"])
    assert r.returncode == 255 and r.stderr.decode() == "IN: Unknown input file format!\n"
    # the VAD module without a name for its decisions: VAD::new_file's words, as in file mode
    r = run(C1 + ["-vad_out_mode", "vad", "-vad_cri_mode", "energy", "-online_in", "-online_out"])
    assert r.returncode == 255 and r.stderr.decode() == "VAD::new_file(): invalid filename!\n"


def test_the_parsers_messages_stand():
    r = run(C1[:3] + ["raw", "-format_out", "wave", "-preset", "exten", "-online_in", "-online_out"])
    assert r.returncode == 255 and r.stderr.decode() == "OPTS: Online output available only for raw and htk formats!\n"
    r = run(C1 + ["-online_in"])
    assert r.returncode == 255 and r.stderr.decode() == "OPTS: Single file mode has to be set at both sides (input and output)!\n"
    r = run(C1 + ["-online_out"])
    assert r.returncode == 255 and r.stderr.decode() == "OPTS: Single file mode has to be set at both sides (input and output)!\n"
