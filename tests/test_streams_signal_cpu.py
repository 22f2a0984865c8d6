"""Stream sets with signal state (CTU_STREAMS_SIGNAL_STATE: speech output on streams), the parts that need no GPU: the exported
symbols, which speech-output configurations such a set takes, which it refuses and with what words, that without the flag every answer
is the one it was, the arithmetic of the samples a stream has delivered against the oracle's output length, and - on the CPU oracle -
the property the feature rests on: the enhancement is causal, so the samples a prefix's frames have completed are those of the whole
file, and only the window - wshift behind them still change.  The planner's signal descriptors are checked by a program of its own
(tests/host/stream_signal_plan_check.cc, tests/test_stream_signal_plan_cpu.py)."""
import ctypes
import itertools

import numpy as np
import pytest

import ctucopy_amd
from ctucopy_amd import streams_config_check, streams_signal_step
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.util import C2, sig, synth_utt

REFUSED = "ENGINE: configuration cannot be streamed: "
SYMBOLS = ("ctu_streams_push_signal", "ctu_streams_push_signal_host", "ctu_streams_finish_signal", "ctu_streams_finish_signal_host",
           "ctu_streams_signal_step")
SIG = "-fs 16000 -format_in raw -format_out raw".split()
PLAIN = ["-nr_mode", "none", "-fea_kind", "none", "-fb_definition", "none"]
A = SIG + ["-preset", "exten"]
B = "-fs 8000 -format_in raw -format_out raw -preset exten".split()
C = SIG + PLAIN + ["-w", "25", "-s", "10", "-preem", "0.97"]
EXTEN_WORDS = REFUSED + "-nr_mode exten (the noise estimate runs from frame to frame of a file)"


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def test_library_exports_and_binding_types_the_new_calls():
    lib = ctypes.CDLL(cbuild.LIB)
    L = ctucopy_amd.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ceng.EXPORTS
        assert getattr(L, name).argtypes, name
    assert L.ctu_streams_signal_step.restype is ctypes.c_int64


def test_the_flag_is_32_and_2_and_16_stay_no_flags():
    assert ceng.STREAMS_SIGNAL_STATE == 32 and 32 & 31 == 0
    assert ceng.STREAMS_SIGNAL_STATE not in (ceng.STREAMS_ROW_STATE, ceng.STREAMS_NR_STATE, ceng.STREAMS_VAD_STATE)
    assert (ceng.STREAMS_ROW_STATE, ceng.STREAMS_NR_STATE, ceng.STREAMS_VAD_STATE) == (1, 4, 8)
    L = ctucopy_amd.load_library()
    buf = ctypes.create_string_buffer(256)
    for cfg in (C2, A):
        n, arr = ceng._argv(cfg)
        for bad in (2, 16, 2 | 32, 16 | 32):
            assert L.ctu_streams_config_check_ex(n, arr, bad, buf, len(buf), None) == ceng.CTU_ERR_INPUT
            assert "unknown stream set flags" in buf.value.decode()


@pytest.mark.parametrize("extra", [["-w", "32", "-s", "16"], ["-w", "25", "-s", "10"], ["-w", "32", "-s", "8"]], ids=["32_16", "25_10", "32_8"])
def test_the_plain_chain_is_taken(extra):
    cfg = SIG + PLAIN + extra
    assert streams_config_check(cfg, signal_state=True) == (ceng.CTU_OK, "")
    assert streams_config_check(cfg, nr_state=True, signal_state=True) == (ceng.CTU_OK, "")
    # the row and the detector flag change nothing on a speech-output configuration
    assert streams_config_check(cfg, row_state=True, vad_state=True, signal_state=True) == (ceng.CTU_OK, "", 0)


@pytest.mark.parametrize("cfg", [A, B, A + ["-nr_a", "1", "-nr_p", "0.9"]], ids=["exten_16k", "exten_8k", "exten_a1_p09"])
def test_exten_is_taken_with_the_noise_state_as_well(cfg):
    assert streams_config_check(cfg, nr_state=True, signal_state=True) == (ceng.CTU_OK, "")
    assert streams_config_check(cfg, row_state=True, nr_state=True, vad_state=True, signal_state=True) == (ceng.CTU_OK, "", 0)
    for kw in ({}, {"row_state": True}, {"vad_state": True}):   # without it: the words exten has on any set
        got = streams_config_check(cfg, signal_state=True, **kw)
        assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[1] == EXTEN_WORDS, got


@pytest.mark.parametrize("cfg, words", [
    ("-fs 16000 -format_in raw -format_out raw -w 25 -s 12.5 -nr_mode fwss -vad burg".split(), ["-nr_mode fwss (the noise estimate"]),
    (SIG + PLAIN + ["-remove_dc1", "on"], ["-remove_dc1 (a frame's offset"]),
    (SIG + PLAIN + ["-w", "40", "-s", "20"], ["-format_out raw | wave", "1024-point"]),
    ("-fs 44100 -format_in raw -format_out raw -w 24 -s 12.5".split() + PLAIN, ["-format_out raw | wave", "2048-point"]),
    ("-fs 44100 -format_in raw -format_out raw -w 24 -s 12.5 -nr_mode exten".split(), ["-format_out raw | wave", "2048-point"]),
], ids=["fwss", "remove_dc1", "1024_points", "2048_points", "2048_points_exten"])
def test_what_a_set_with_signal_state_still_refuses_by_name(cfg, words):
    for kw in ({"nr_state": True}, {"nr_state": True, "vad_state": True}, {"row_state": True, "nr_state": True}):
        got = streams_config_check(cfg, signal_state=True, **kw)
        assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[1].startswith(REFUSED), got
        for w in words:
            assert w in got[1], got
    if "exten" not in cfg:   # (exten without the noise state is refused as exten, whatever follows)
        got = streams_config_check(cfg, signal_state=True)
        assert got[0] == ceng.CTU_ERR_UNSUPPORTED and all(w in got[1] for w in words), got


def test_remove_dc1_behind_exten_is_refused_as_remove_dc1_once_the_noise_state_is_there():
    cfg = A + ["-remove_dc1", "on"]
    assert streams_config_check(cfg, signal_state=True) == (ceng.CTU_ERR_UNSUPPORTED, EXTEN_WORDS)
    got = streams_config_check(cfg, nr_state=True, signal_state=True)
    assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[1].startswith(REFUSED + "-remove_dc1 (a frame's offset"), got


SPEECH = {"exten_16k": A, "exten_8k": B, "plain_25_10": C, "plain_1024": SIG + PLAIN + ["-w", "40", "-s", "20"],
          "fwss": "-fs 16000 -format_in raw -format_out raw -w 25 -s 12.5 -nr_mode fwss -vad burg".split()}


@pytest.mark.parametrize("name", list(SPEECH))
def test_without_the_flag_speech_output_is_refused_with_the_words_it_had(name):
    cfg = SPEECH[name]
    today = streams_config_check(cfg)
    assert today == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-format_out raw | wave (speech output: the overlap-add runs across a file's frames)")
    L = ctucopy_amd.load_library()
    n, arr = ceng._argv(cfg)
    for flags in sorted({a | b | c for a, b, c in itertools.product((0, 1), (0, 4), (0, 8))}):
        buf = ctypes.create_string_buffer(1024)
        halo = ctypes.c_int32(-1)
        assert L.ctu_streams_config_check_ex(n, arr, flags, buf, len(buf), ctypes.byref(halo)) == today[0], flags
        assert buf.value.decode() == today[1] and halo.value == 0, flags


@pytest.mark.parametrize("cfg", [C2, C2 + ["-nr_mode", "exten"], C2 + ["-fea_delta", "d_a"], C2 + ["-w", "40"], "-fs 16000 -bogus 1".split()],
                         ids=["mfcc", "mfcc_exten", "d_a", "1024", "bad_option"])
def test_on_a_configuration_without_speech_output_the_flag_changes_nothing(cfg):
    assert streams_config_check(cfg, signal_state=True) == streams_config_check(cfg)
    assert streams_config_check(cfg, row_state=True, signal_state=True) == streams_config_check(cfg, row_state=True)
    assert streams_config_check(cfg, nr_state=True, signal_state=True) == streams_config_check(cfg, nr_state=True)


# (window, wshift) -> a plain speech-output chain at 16 kHz with that frame shape
SHAPES = {(512, 256): ["-w", "32", "-s", "16"], (256, 128): ["-w", "16", "-s", "8"], (400, 160): ["-w", "25", "-s", "10"],
          (512, 128): ["-w", "32", "-s", "8"], (400, 161): ["-w", "25", "-s", "10.0625"]}


@pytest.mark.parametrize("shape", list(SHAPES), ids=["%d_%d" % s for s in SHAPES])
def test_signal_step_is_the_oracles_output_length_sample_by_sample(shape):
    w, s = shape
    orc = Oracle(SIG + PLAIN + SHAPES[shape])
    n_max = 3 * w + 5 * s
    x = synth_utt(17, n_max)
    lengths = {}   # the oracle's output length depends on the frame count alone: one run per count
    for n in range(n_max + 1):
        T = orc.num_frames(n)
        delivered, pending = streams_signal_step(w, s, n)
        if T > 0:
            if T not in lengths:
                lengths[T] = len(orc.enhance(x[:n]))
                assert lengths[T] == T * s + w - s
            assert delivered + pending == lengths[T], n
            assert delivered == s * T and pending == w - s, n
        else:
            assert (delivered, pending) == (0, 0), n
    assert len(lengths) >= 6
    assert ctucopy_amd.load_library().ctu_streams_signal_step(w, s, -1, None) == ceng.CTU_ERR_INPUT
    assert ctucopy_amd.load_library().ctu_streams_signal_step(s, w, 5, None) == ceng.CTU_ERR_INPUT


@pytest.mark.parametrize("cfg", [A, C], ids=["exten_16k", "plain_25_10"])
def test_the_reference_is_causal_a_prefix_has_the_whole_files_samples(cfg):
    orc = Oracle(cfg)
    w, s = (512, 256) if cfg is A else (400, 160)
    x = sig("CS0")[:w + 95 * s + s // 2].copy()
    assert orc.num_frames(x.size) == 96
    cut = w + 40 * s + 13   # 41 frames and a few samples that complete none
    assert orc.num_frames(cut) == 41
    whole, prefix = orc.enhance(x), orc.enhance(x[:cut])
    assert whole.size == 96 * s + w - s and prefix.size == 41 * s + w - s
    assert np.array_equal(prefix[:41 * s], whole[:41 * s])
    assert not np.array_equal(prefix[41 * s:], whole[41 * s:41 * s + w - s])
