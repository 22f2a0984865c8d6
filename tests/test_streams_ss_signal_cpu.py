"""Stream sets with subtraction state and signal state in one set (CTU_STREAMS_SS_SIGNAL_STATE beside CTU_STREAMS_SS_STATE and
CTU_STREAMS_SIGNAL_STATE: the speech output of -nr_mode hwss | fwss | 2fwss on streams), the parts that need no GPU: the flag's value
and that it is a flag only beside both of the others, which configurations such a set takes, what it refuses by name, that what the
engine itself refuses keeps the engine's words, that without the flag every answer keeps the words it had and that beside another
configuration the flag changes no answer; and - on the CPU oracle - the rule the feature rests on (the enhancement is causal: a
prefix's completed frames give the whole file's samples) and that the inputs of tests/test_streams_ss_signal.py make the detector take
both decisions behind the initial segments.

The answers "without the flag" are written out here from the sentences tests/test_streams_ss_cpu.py and tests/test_streams_signal_cpu.py
hold, not taken from the code under test."""
import ctypes
import itertools

import numpy as np
import pytest

import ctucopy_amd
from ctucopy_amd import streams_config_check
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.util import C2, C5, sig, synth_utt

SS, SIGNAL, BOTH = 1024, 32, 2048
ALL3 = SS | SIGNAL | BOTH
EVERY = ALL3 | 1 | 4 | 8 | 64 | 256
UNKNOWN = (ceng.CTU_ERR_INPUT, "ENGINE: unknown stream set flags")
REFUSED = "ENGINE: configuration cannot be streamed: "
NOT_ACCELERATED = "ENGINE: configuration not on the accelerated path: "
SIG_FWSS = "-fs 16000 -format_in raw -format_out raw -w 25 -s 12.5 -nr_mode fwss -vad burg".split()   # tests/util.py: sig_fwss
SS8 = "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97 -vad burg".split()
FWSS = ["-nr_mode", "fwss"]


def _speech(mode, fs=16000, extra=()):
    return f"-fs {fs} -format_in raw -format_out raw -w 25 -s 12.5 -nr_mode {mode} -vad burg".split() + list(extra)


TAKEN = {
    "fwss_16k": SIG_FWSS, "2fwss_16k": _speech("2fwss"), "hwss_16k": _speech("hwss"),
    "fwss_8k": _speech("fwss", 8000), "2fwss_8k": _speech("2fwss", 8000), "hwss_8k": _speech("hwss", 8000),
    "w20_s10": SIG_FWSS + ["-w", "20", "-s", "10"], "w25_s10": SIG_FWSS + ["-s", "10"],
    "ncep5": SIG_FWSS + ["-fea_ncepcoefs", "5"], "ncep16": SIG_FWSS + ["-fea_ncepcoefs", "16"],
    "nr_a2": SIG_FWSS + ["-nr_a", "2"], "wave": SIG_FWSS[:4] + ["-format_out", "wave"] + SIG_FWSS[6:],
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def _check(cfg, flags):
    L = ctucopy_amd.load_library()
    n, arr = ceng._argv(cfg)
    buf = ctypes.create_string_buffer(2048)
    halo = ctypes.c_int32(-1)
    rc = L.ctu_streams_config_check_ex(n, arr, flags, buf, len(buf), ctypes.byref(halo))
    return int(rc), buf.value.decode(), int(halo.value)


def _subsets(bits):
    return [sum(c) for k in range(len(bits) + 1) for c in itertools.combinations(bits, k)]


def _mode(cfg):
    return cfg[cfg.index("-nr_mode") + 1]


def _parent_answer(cfg, flags):
    """What a set answered to a speech-output *ss configuration before the flag existed (flags without 2048 and without 64)."""
    mode = _mode(cfg)
    if flags & SS:   # tests/test_streams_ss_cpu.py: speech_output, speech_output_signal_flag
        why = "-nr_mode %s with -format_out raw | wave (speech output behind hwss / fwss / 2fwss is not streamed, whatever the signal flag: the subtraction state serves the feature path)" % mode
    elif not flags & SIGNAL:   # tests/test_streams_signal_cpu.py: test_without_the_flag_speech_output_is_refused_with_the_words_it_had
        why = "-format_out raw | wave (speech output: the overlap-add runs across a file's frames)"
    else:   # tests/test_streams_signal_cpu.py: test_what_a_set_with_signal_state_still_refuses_by_name[fwss]
        why = "-nr_mode %s (the noise estimate runs from frame to frame of a file)" % mode
    return ceng.CTU_ERR_UNSUPPORTED, REFUSED + why, 0


def test_the_flag_is_2048_and_a_flag_only_beside_both_states():
    assert ceng.STREAMS_SS_SIGNAL_STATE == BOTH == 2048
    assert (ceng.STREAMS_ROW_STATE, ceng.STREAMS_NR_STATE, ceng.STREAMS_VAD_STATE, ceng.STREAMS_SIGNAL_STATE, ceng.STREAMS_LARGE_STATE,
            ceng.STREAMS_TRAP_STATE, ceng.STREAMS_SS_STATE) == (1, 4, 8, 32, 64, 256, 1024)
    for cfg in (C2, SIG_FWSS, SS8 + FWSS):
        for flags in (BOTH, BOTH | SS, BOTH | SIGNAL, BOTH | SS | 1, BOTH | SIGNAL | 4 | 8 | 256):
            assert _check(cfg, flags)[:2] == UNKNOWN, (cfg, flags)
        assert "unknown stream set flags" not in _check(cfg, ALL3)[1], cfg
        assert "unknown stream set flags" not in _check(cfg, EVERY)[1], cfg
        for bad in (2, 16, 128, 512, 4096):
            assert _check(cfg, bad)[:2] == UNKNOWN, (cfg, bad)
            assert _check(cfg, bad | ALL3)[:2] == UNKNOWN, (cfg, bad)


def test_the_binding_carries_the_flag_last():
    assert ceng._stream_flags(True, True, True, True, True, True, True) == 1 | 4 | 8 | 32 | 64 | 256 | 1024   # the seven-argument call is what it was
    assert ceng._stream_flags(True, True, True, True, True, True, True, True) == EVERY
    assert ceng._stream_flags(signal_state=True, ss_state=True, ss_signal_state=True) == ALL3
    assert streams_config_check(SIG_FWSS, signal_state=True, ss_state=True, ss_signal_state=True) == (ceng.CTU_OK, "")
    assert streams_config_check(SIG_FWSS, False, False, False, True, False, False, True, True) == (ceng.CTU_OK, "")
    assert streams_config_check(SIG_FWSS, ss_signal_state=True) == UNKNOWN
    assert streams_config_check(SIG_FWSS, signal_state=True, ss_state=True) == _parent_answer(SIG_FWSS, SS | SIGNAL)[:2]


@pytest.mark.parametrize("name", list(TAKEN))
def test_the_modes_with_speech_output_are_taken_with_the_three_flags_and_no_halo(name):
    cfg = TAKEN[name]
    assert _check(cfg, ALL3) == (ceng.CTU_OK, "", 0)
    assert _check(cfg, EVERY) == (ceng.CTU_OK, "", 0)   # ... whatever other flags come with them
    for flags in _subsets([1, 4, 8, 256]):
        assert _check(cfg, ALL3 | flags) == (ceng.CTU_OK, "", 0), flags


@pytest.mark.parametrize("name", list(TAKEN))
def test_without_the_flag_every_answer_is_the_sentence_it_was(name):
    cfg = TAKEN[name]
    for flags in _subsets([1, 4, 8, 32, 256, 1024]):
        assert _check(cfg, flags) == _parent_answer(cfg, flags), flags


@pytest.mark.parametrize("cfg, word", [
    (SIG_FWSS[:-1] + ["file=dec.bin"], "-vad file=... with -nr_mode fwss (the decision bytes are one stream per process"),
    ("-fs 44100 -format_in raw -format_out raw -w 24 -s 12.5 -nr_mode hwss -vad burg".split(), "-nr_mode hwss on 2048-point frames (-w: the passes of the large transforms' subtraction are not streamed"),
    ("-fs 48000 -format_in raw -format_out raw -w 64 -s 16 -nr_mode 2fwss -vad burg".split(), "-nr_mode 2fwss on 4096-point frames"),
    (SIG_FWSS + ["-s", "30"], "-s above -w (frames that leave samples out)"),
], ids=["vad_file", "hwss_2048", "2fwss_4096", "s_above_w"])
def test_what_is_refused_with_the_flags_is_refused_by_name(cfg, word):
    for flags in (ALL3, EVERY):
        rc, why, halo = _check(cfg, flags)
        assert rc == ceng.CTU_ERR_UNSUPPORTED and halo == 0 and why.startswith(REFUSED + word), why
    assert _check(cfg, SS | SIGNAL) == _parent_answer(cfg, SS | SIGNAL)


@pytest.mark.parametrize("cfg, word", [
    (SIG_FWSS + ["-remove_dc1", "on"], "hwss / fwss / 2fwss with signal output outside the detector paths"),
    (SIG_FWSS + ["-w", "30"], "hwss / fwss / 2fwss with signal output outside the detector paths"),
    (_speech("fwss", 8000, ["-w", "30"]), "hwss / fwss / 2fwss with signal output outside the detector paths"),
    (SIG_FWSS + ["-vad_out_mode", "vad"], "signal output"),
], ids=["remove_dc1", "w30_16k", "w30_8k", "vad_module"])
def test_what_the_engine_refuses_keeps_the_engine_s_words(cfg, word):
    got = _check(cfg, ALL3)
    assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[2] == 0 and got[1].startswith(NOT_ACCELERATED) and word in got[1], got
    for flags in (0, SIGNAL, SS | SIGNAL, EVERY):
        assert _check(cfg, flags) == got, flags


@pytest.mark.parametrize("cfg", [C2, C2 + ["-nr_mode", "exten"], C5, "-fs 16000 -format_in raw -format_out raw -preset exten".split(), SS8 + FWSS],
                         ids=["C2", "C2_exten", "C5", "SIG_EXTEN", "SS8_FWSS"])
def test_beside_another_configuration_the_flag_changes_no_answer(cfg):
    for flags in _subsets([1, 4, 8, 256]) + [64, 64 | 4, 64 | 4 | 1 | 8 | 256]:
        assert _check(cfg, flags | ALL3) == _check(cfg, flags | SS | SIGNAL), flags
    assert "unknown" not in _check(cfg, ALL3)[1]


# ---- on the oracle

CASES = {   # the configurations and inputs of tests/test_streams_ss_signal.py: (configuration, 96 frames and a few samples that complete none)
    "fwss_16k": (_speech("fwss"), lambda n: sig("CS0")[:n].copy()),
    "hwss_16k": (_speech("hwss"), lambda n: sig("CS0")[:n].copy()),
    "2fwss_16k": (_speech("2fwss"), lambda n: sig("CS0")[:n].copy()),
    "fwss_8k": (_speech("fwss", 8000), lambda n: synth_utt(5, n, fs=8000)),
    "2fwss_8k": (_speech("2fwss", 8000, ["-nr_p", "0.9", "-nr_q", "0.95"]), lambda n: synth_utt(5, n, fs=8000)),
    "hwss_8k": (_speech("hwss", 8000), lambda n: synth_utt(5, n, fs=8000)),
    "fwss_8k_a2_ncep5": (_speech("fwss", 8000, ["-nr_a", "2", "-fea_ncepcoefs", "5"]), lambda n: synth_utt(5, n, fs=8000)),
    "fwss_16k_s10": (_speech("fwss", 16000, ["-s", "10"]), lambda n: sig("CS0")[:n].copy()),
}


def _shape(cfg):
    fs = int(cfg[1])
    s = 10.0 if cfg[-2:] == ["-s", "10"] else 12.5
    return fs * 25 // 1000, int(fs * s / 1000)


def case_input(name, frames=96):
    cfg, make = CASES[name]
    w, s = _shape(cfg)
    return cfg, make(w + (frames - 1) * s + s // 2)


@pytest.mark.parametrize("name", ["fwss_16k", "2fwss_8k"])
def test_the_reference_is_causal_a_prefix_has_the_whole_files_samples(name):
    cfg, x = case_input(name)
    w, s = _shape(cfg)
    assert Oracle(cfg).num_frames(x.size) == 96
    cut = w + 40 * s + 13   # 41 frames and a few samples that complete none
    assert Oracle(cfg).num_frames(cut) == 41
    whole, prefix = Oracle(cfg).enhance(x), Oracle(cfg).enhance(x[:cut])   # a fresh oracle per file: every file is a first file
    assert whole.size == 96 * s + w - s and prefix.size == 41 * s + w - s
    assert np.array_equal(prefix[:41 * s], whole[:41 * s])


@pytest.mark.parametrize("name", list(CASES))
def test_the_inputs_of_the_gpu_tests_make_the_detector_take_both_decisions(name, tmp_path):
    """A condition on the inputs: under -vad burg the samples differ from those under decisions that are all zeros and from those
    under decisions that are all ones, somewhere behind frame nr_initsegs - so the detector says both, and the gated update runs."""
    cfg, x = case_input(name)
    w, s = _shape(cfg)
    burg = Oracle(cfg).enhance(x)
    init = 10   # -nr_initsegs' default (the frames whose update no decision gates)
    for byte in (0, 1):
        f = tmp_path / ("dec%d.bin" % byte)
        f.write_bytes(bytes(np.full(96, byte, np.uint8)))
        at = cfg.index("-vad") + 1
        forced = Oracle(cfg[:at] + ["file=%s" % f] + cfg[at + 1:]).enhance(x)
        assert forced.shape == burg.shape
        # (frame t reaches the samples [t s, t s + w): those from init s + w on come from frames behind nr_initsegs alone)
        assert not np.array_equal(forced[init * s + w:], burg[init * s + w:]), (name, byte)
