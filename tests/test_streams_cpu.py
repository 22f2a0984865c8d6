"""Streaming input (ctu_streams_*), the parts that need no GPU: the exported symbols, which configurations a stream set refuses and
with what words, and the frame / carry arithmetic of a stream against the oracle's frame count."""
import ctypes

import pytest

import ctucopy_amd
from ctucopy_amd import CtuError, config_dims, streams_config_check, streams_step
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.util import C2, C3

C2_8K = "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97".split()
SYMBOLS = ("ctu_streams_create", "ctu_streams_destroy", "ctu_streams_push", "ctu_streams_push_host", "ctu_streams_finish",
           "ctu_streams_frames")


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def test_library_exports_the_stream_calls():
    lib = ctypes.CDLL(cbuild.LIB)
    for name in SYMBOLS + ("ctu_streams_config_check", "ctu_streams_step", "ctu_streams_last_push_ms"):
        assert hasattr(lib, name), name


def test_binding_resolves_the_stream_calls():
    L = ctucopy_amd.load_library()
    for name in SYMBOLS:
        assert name in ceng.EXPORTS
        assert getattr(L, name).argtypes, name
    assert L.ctu_streams_frames.restype is ctypes.c_int64
    assert callable(ctucopy_amd.Engine.streams) and callable(ctucopy_amd.Streams.push) and callable(ctucopy_amd.Streams.finish)


def test_no_device_no_engine_and_so_no_stream_set():
    import torch
    if torch.cuda.is_available():
        return  # (with a GPU this is tests/test_streams.py's ground)
    with pytest.raises(CtuError) as ei:
        ctucopy_amd.Engine(C2)
    assert ei.value.code == ceng.CTU_ERR_DEVICE


@pytest.mark.parametrize("cfg", [C2, C3, C2_8K, C2 + ["-w", "40"], C2 + ["-w", "100"],
                                 C2_8K + ["-w", "8", "-s", "4", "-fb_definition", "1-10/10filters", "-fea_ncepcoefs", "8"], C2 + ["-fea_kind", "logspec", "-fea_E", "on"], C2 + ["-fea_E", "on", "-fea_rawenergy", "on"],
                                 C2 + ["-fb_definition", "40filters", "-fea_ncepcoefs", "39"], C2 + ["-s", "10.0625"],
                                 C2 + ["-remove_dc", "off"], C3 + ["-fea_kind", "lpa"]])
def test_stateless_chains_are_streamable(cfg):
    assert streams_config_check(cfg) == (ceng.CTU_OK, "")


@pytest.mark.parametrize("extra, word", [
    (["-nr_mode", "exten"], "-nr_mode exten"),
    (["-fea_delta", "d_a"], "-fea_delta"),
    (["-fea_trap", "5"], "-fea_trap"),
    (["-fea_Z_exp", "500"], "-fea_Z_exp"),
    (["-fea_Z_block", "500"], "-fea_Z_block"),
    (["-vad_out_mode", "vad", "-vad_out", "x.vad"], "VAD module"),
    (["-vad_apply_mode", "silence"], "VAD module"),
    (["-remove_dc1", "on"], "-remove_dc1"),
    (["-fb_definition", "23filters", "-fea_kind", "trapdct,101,16"], "trapdct"),
    (["-stat_cmvn", "stat.txt"], "-stat_cmvn"),
])
def test_chains_with_state_across_frames_are_refused_by_name(extra, word):
    rc, why = streams_config_check(C2 + extra)
    assert rc == ceng.CTU_ERR_UNSUPPORTED
    assert why.startswith("ENGINE: configuration cannot be streamed: ") and word in why, why


def test_speech_output_and_feature_input_are_refused_by_name():
    rc, why = streams_config_check("-fs 16000 -format_in raw -format_out raw -preset exten".split())
    assert rc == ceng.CTU_ERR_UNSUPPORTED and "cannot be streamed" in why and "-format_out raw | wave" in why, why
    rc, why = streams_config_check("-fs 16000 -format_in htk -format_out htk -preset mfcc -fea_rawenergy on -nfeacoefs 13".split())
    assert rc == ceng.CTU_ERR_UNSUPPORTED and "cannot be streamed" in why and "-format_in htk" in why, why


def test_what_the_engine_refuses_keeps_the_engine_s_words():
    rc, why = streams_config_check(C2 + ["-dither", "1.0"])
    assert rc == ceng.CTU_ERR_UNSUPPORTED and why.startswith("ENGINE: configuration not on the accelerated path: ") and "-dither" in why
    rc, why = streams_config_check("-fs 16000 -bogus 1".split())
    assert rc == ceng.CTU_ERR_OPTS and "Syntax error" in why


@pytest.mark.parametrize("cfg", [C2, C2_8K, C2 + ["-s", "10.0625"]])
def test_frame_and_carry_arithmetic_against_the_oracle(cfg):
    d = config_dims(cfg)
    w, s = d.window, d.wshift
    orc = Oracle(cfg)
    totals = [0, 1, w - s - 1, w - s, w - 1, w, w + 1, w + s - 1, w + s, w + 7 * s, 10 * s + 3, 100 * w + 17]
    for n in totals:
        frames, carry = streams_step(w, s, n)
        assert frames == max(orc.num_frames(n), 0), n       # a file too short for the reference (-1) has produced no frame yet
        assert carry == n - frames * s and 0 <= carry < w, n  # what the next frame already has never fills a window
    # the count after a push does not depend on how the samples came: one sample at a time is the extreme
    total = 0
    for _ in range(3 * w):
        total += 1
        assert streams_step(w, s, total)[0] == max(orc.num_frames(total), 0)
    for bad in ((0, 1, 5), (400, 0, 5), (400, 401, 5), (400, 160, -1)):
        with pytest.raises(CtuError):
            streams_step(*bad)
