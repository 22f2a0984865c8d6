"""Stream sets with subtraction state on large transforms (CTU_STREAMS_SS_LARGE_STATE beside CTU_STREAMS_SS_STATE: -nr_mode hwss | fwss |
2fwss with -vad burg on the feature path of 2048- and 4096-point frames), the parts that need no GPU: the flag's value and that it is a
flag only beside the subtraction state, which configurations such a set takes, what it refuses by name, that what the engine itself
refuses keeps the engine's words, that without the flag every answer keeps the words it had and that beside another configuration the
flag changes no answer.

The answers "without the flag" are written out here from the sentences tests/test_streams_ss_cpu.py and
tests/test_streams_ss_signal_cpu.py hold, not taken from the code under test."""
import ctypes
import inspect
import itertools

import pytest

import ctucopy_amd
from ctucopy_amd import streams_config_check
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from tests.test_ss_big_cpu import B, K1024, M, SIGNAL_CONFIGS, W64
from tests.util import C2, C5

SS, LARGE = 1024, 8192
BOTH = SS | LARGE
HARMLESS = [1, 4, 8, 32, 64, 256, 2048]   # (64 is a flag beside 4 or 32 only, 2048 beside 1024 and 32 only)
EVERY = BOTH | 1 | 4 | 8 | 32 | 64 | 256 | 2048
UNKNOWN = (ceng.CTU_ERR_INPUT, "ENGINE: unknown stream set flags")
REFUSED = "ENGINE: configuration cannot be streamed: "
NOT_ACCELERATED = "ENGINE: configuration not on the accelerated path: "
SS8_FWSS = "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97 -vad burg -nr_mode fwss".split()

TAKEN = {   # (tests/test_streams_ss_large.py runs these on the GPU)
    "fwss_44k": M(44100) + B + ["-nr_mode", "fwss"],
    "2fwss_44k_p_q": M(44100) + B + ["-nr_mode", "2fwss", "-nr_p", "0.9", "-nr_q", "0.95"],
    "hwss_spec_44k_a2_b15": M(44100) + B + ["-nr_mode", "hwss", "-fea_kind", "spec", "-nr_a", "2", "-nr_b", "1.5"],
    "fwss_44k_ncep20": M(44100) + B + ["-nr_mode", "fwss", "-fea_kind", "logspec", "-fea_ncepcoefs", "20"],
    "fwss_44k_lpc": M(44100) + B + ["-nr_mode", "fwss", "-fea_kind", "lpc", "-fea_lporder", "12", "-fb_inld", "on", "-fb_eqld", "on"],
    "fwss_44k_E": M(44100) + B + ["-nr_mode", "fwss", "-fea_E", "on"],
    "fwss_48k_w64": M(48000) + W64 + B + ["-nr_mode", "fwss"],
}
CHAIN = M(44100) + B + ["-nr_mode", "2fwss", "-fea_delta", "d_a", "-fea_Z_exp", "500"]   # halo 2 + 2


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


def _known(flags):
    """The rules of the flags that say how far another reaches (include/ctu_engine.h), without 8192."""
    return not (flags & 64 and not flags & (4 | 32)) and not (flags & 2048 and flags & (1024 | 32) != (1024 | 32))


def _mode(cfg):
    return cfg[cfg.index("-nr_mode") + 1]


def _points(cfg):
    return 4096 if "48000" in cfg else 2048


def _parent_answer(cfg, flags):
    """What a set answered to a *ss configuration on the feature path of 2048- / 4096-point frames before the flag existed."""
    if flags & SS:   # tests/test_streams_ss_cpu.py, tests/test_streams_ss_signal_cpu.py: hwss_2048, 2fwss_4096
        why = ("-nr_mode %s on %d-point frames (-w: the passes of the large transforms' subtraction are not streamed, a stream set carries the one "
               "of the 256- and 512-point front end)" % (_mode(cfg), _points(cfg)))
    else:   # tests/test_streams_ss_cpu.py: test_without_the_flag_every_answer_is_the_sentence_it_was
        why = "-nr_mode %s (the noise estimate runs from frame to frame of a file)" % _mode(cfg)
    return ceng.CTU_ERR_UNSUPPORTED, REFUSED + why, 0


def test_the_flag_is_8192():
    assert ceng.STREAMS_SS_LARGE_STATE == LARGE == 8192
    assert (ceng.STREAMS_ROW_STATE, ceng.STREAMS_NR_STATE, ceng.STREAMS_VAD_STATE, ceng.STREAMS_SIGNAL_STATE, ceng.STREAMS_LARGE_STATE,
            ceng.STREAMS_TRAP_STATE, ceng.STREAMS_SS_STATE, ceng.STREAMS_SS_SIGNAL_STATE) == (1, 4, 8, 32, 64, 256, 1024, 2048)


def test_the_tile_length_can_be_asked():
    """tests/test_streams_ss_large.py sizes its push across a tile edge by it."""
    for cfg in (C2, TAKEN["fwss_44k"], TAKEN["fwss_48k_w64"]):
        t = ctucopy_amd.config_table(cfg, "tile_frames")
        assert t.shape == (1,) and t[0] == int(t[0]) and t[0] >= 8


@pytest.mark.parametrize("cfg", [C2, TAKEN["fwss_44k"], SS8_FWSS], ids=["C2", "fwss_44k", "fwss_8k"])
def test_it_is_a_flag_only_beside_the_subtraction_state_and_4096_is_none(cfg):
    assert _check(cfg, LARGE)[:2] == UNKNOWN
    for flags in _subsets(HARMLESS):
        assert _check(cfg, LARGE | flags)[:2] == UNKNOWN, flags   # without 1024
        assert _check(cfg, 4096 | flags)[:2] == UNKNOWN, flags    # 4096 in any company
        assert _check(cfg, 4096 | BOTH | flags)[:2] == UNKNOWN, flags
        assert _check(cfg, 4096 | SS | flags)[:2] == UNKNOWN, flags
    for flags in _subsets([1, 4, 8, 32, 256]):
        assert "unknown stream set flags" not in _check(cfg, BOTH | flags)[1], flags
    assert "unknown stream set flags" not in _check(cfg, EVERY)[1]
    for bad in (2, 16, 128, 512):
        assert _check(cfg, bad | EVERY)[:2] == UNKNOWN, bad
    assert _check(cfg, BOTH | 64)[:2] == UNKNOWN   # it does not involve 64: 64 | 1024 stays unknown, with 8192 as without
    assert _check(cfg, SS | 64)[:2] == UNKNOWN


def test_the_binding_carries_the_keyword_last():
    assert ceng._stream_flags(True, True, True, True, True, True, True, True) == 1 | 4 | 8 | 32 | 64 | 256 | 1024 | 2048   # the eight-argument call is what it was
    assert ceng._stream_flags(True, True, True, True, True, True, True, True, True) == EVERY
    assert ceng._stream_flags(ss_state=True, ss_large_state=True) == BOTH
    for f in (ceng._stream_flags, ceng.streams_config_check, ceng.Streams.__init__, ceng.Engine.streams):
        last = list(inspect.signature(f).parameters.values())[-1]
        assert last.name == "ss_large_state" and last.default is False, f
    cfg = TAKEN["fwss_44k"]
    assert streams_config_check(cfg, ss_state=True, ss_large_state=True) == (ceng.CTU_OK, "")
    assert streams_config_check(cfg, False, False, False, False, False, False, True, False, True) == (ceng.CTU_OK, "")
    assert streams_config_check(cfg, ss_large_state=True) == UNKNOWN
    assert streams_config_check(cfg, ss_state=True) == _parent_answer(cfg, SS)[:2]
    assert streams_config_check(CHAIN, row_state=True, ss_state=True, ss_large_state=True) == (ceng.CTU_OK, "", 4)


@pytest.mark.parametrize("name", list(TAKEN))
def test_the_modes_are_taken_on_2048_and_4096_points_with_the_two_flags_and_no_halo(name):
    cfg = TAKEN[name]
    assert _check(cfg, BOTH) == (ceng.CTU_OK, "", 0)
    assert _check(cfg, EVERY) == (ceng.CTU_OK, "", 0)   # ... whatever harmless flags come with them
    for flags in _subsets(HARMLESS):
        if _known(flags | SS):
            assert _check(cfg, BOTH | flags) == (ceng.CTU_OK, "", 0), flags


def test_a_chain_behind_them_needs_the_row_state():
    assert _check(CHAIN, BOTH | 1) == (ceng.CTU_OK, "", 4)
    assert _check(CHAIN, EVERY) == (ceng.CTU_OK, "", 4)
    assert _check(CHAIN, BOTH) == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-fea_delta (the delta chain spans the frames of its windows)", 0)
    cms = TAKEN["fwss_44k"] + ["-fea_Z_exp", "500"]
    assert _check(cms, BOTH | 1) == (ceng.CTU_OK, "", 0)
    assert _check(cms, BOTH) == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-fea_Z_exp (CMS: the running mean runs along the file)", 0)


@pytest.mark.parametrize("name", list(TAKEN) + ["chain"])
def test_without_the_flag_every_answer_is_the_sentence_it_was(name):
    cfg = CHAIN if name == "chain" else TAKEN[name]
    for flags in _subsets([1, 4, 8, 32, 256, 1024]):
        assert _check(cfg, flags) == _parent_answer(cfg, flags), flags
        for beside in (4, 32):   # 64 is a flag beside either
            assert _check(cfg, flags | beside | 64) == _parent_answer(cfg, flags), (flags, beside)
    assert _check(cfg, SS | 32 | 2048) == _parent_answer(cfg, SS)
    assert _check(cfg, BOTH | 1)[:2] == (ceng.CTU_OK, "")   # ... and with it the configuration is taken


def test_1024_4_64_on_a_2048_point_2fwss_configuration_is_what_it_was():
    cfg = M(44100) + B + ["-nr_mode", "2fwss"]
    assert _check(cfg, 1024 | 4 | 64) == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-nr_mode 2fwss on 2048-point frames (-w: the passes of the large transforms' "
                                          "subtraction are not streamed, a stream set carries the one of the 256- and 512-point front end)", 0)
    assert _check(cfg, 1024 | 4 | 64 | LARGE) == (ceng.CTU_OK, "", 0)


@pytest.mark.parametrize("cfg", [C2, C2 + ["-nr_mode", "exten"], C2 + ["-nr_mode", "exten", "-fea_delta", "d_a"], C5, SS8_FWSS, M(44100), M(44100) + ["-nr_mode", "exten"]],
                         ids=["C2", "C2_exten", "C2_exten_d_a", "C5", "SS8_FWSS", "M44", "M44_exten"])
def test_beside_another_configuration_the_flag_changes_no_answer(cfg):
    for flags in _subsets([1, 4, 8, 32, 256]) + [64 | 4, 64 | 32, 2048 | 32, 64 | 4 | 1 | 8 | 256 | 32 | 2048]:
        assert _check(cfg, flags | BOTH) == _check(cfg, flags | SS), flags
    assert "unknown" not in _check(cfg, BOTH)[1]


@pytest.mark.parametrize("cfg, word", [
    (M(44100) + ["-vad", "file=dec.bin", "-nr_mode", "fwss"], "-vad file=... with -nr_mode fwss (the decision bytes are one stream per process"),
    (M(48000) + W64 + ["-vad", "file=dec.bin", "-nr_mode", "2fwss"], "-vad file=... with -nr_mode 2fwss (the decision bytes are one stream per process"),
    (SIGNAL_CONFIGS[0], "-nr_mode fwss with -format_out raw | wave on 2048-point frames (speech output behind the large transforms' subtraction is not streamed"),
    (SIGNAL_CONFIGS[1], "-nr_mode 2fwss with -format_out raw | wave on 4096-point frames (speech output behind the large transforms' subtraction is not streamed"),
    (M(44100) + B + ["-nr_mode", "fwss", "-s", "30"], "-s above -w (frames that leave samples out)"),
], ids=["vad_file_2048", "vad_file_4096", "speech_2048", "speech_4096", "s_above_w"])
def test_what_is_refused_with_the_flag_is_refused_by_name(cfg, word):
    for flags in (BOTH, BOTH | 32, BOTH | 32 | 2048, BOTH | 1 | 4 | 64, EVERY):   # (EVERY: every flag set)
        rc, why, halo = _check(cfg, flags)
        assert rc == ceng.CTU_ERR_UNSUPPORTED and halo == 0 and why.startswith(REFUSED + word), (flags, why)


@pytest.mark.parametrize("cfg", SIGNAL_CONFIGS, ids=["speech_2048", "speech_4096"])
def test_speech_output_without_the_flag_is_refused_with_the_words_it_had(cfg):
    mode, n = _mode(cfg), _points(cfg)
    plain = REFUSED + "-nr_mode %s with -format_out raw | wave (speech output behind hwss / fwss / 2fwss is not streamed, whatever the signal flag: the subtraction state serves the feature path)" % mode
    sized = REFUSED + "-nr_mode %s on %d-point frames (-w: the passes of the large transforms' subtraction are not streamed" % (mode, n)
    assert _check(cfg, SS)[:2] == (ceng.CTU_ERR_UNSUPPORTED, plain)
    assert _check(cfg, SS | 32)[:2] == (ceng.CTU_ERR_UNSUPPORTED, plain)
    got = _check(cfg, SS | 32 | 2048)   # tests/test_streams_ss_signal_cpu.py: hwss_2048, 2fwss_4096
    assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[1].startswith(sized), got
    assert _check(cfg, 32)[:2] == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-nr_mode %s (the noise estimate runs from frame to frame of a file)" % mode)
    assert _check(cfg, BOTH)[1] not in (plain, got[1]) and _check(cfg, BOTH)[1].startswith(REFUSED)   # with the flag: a sentence of its own


@pytest.mark.parametrize("name, frames, init", [("fwss_44k", 44, 10), ("2fwss_44k_p_q", 44, 10), ("fwss_48k_w64", 44, 10), ("fwss_44k", 12, 2)])
def test_the_inputs_of_the_gpu_tests_make_the_detector_take_both_decisions(name, frames, init, tmp_path):
    """A condition on the inputs of tests/test_streams_ss_large.py (file 1 of the list of tests/test_ss_big.py, cut to `frames` frames;
    the 12-frame input is one of the four that run under -nr_initsegs 2 there): on the CPU oracle the rows under -vad burg differ from those under decisions that
    are all zeros and from those under decisions that are all ones, somewhere behind frame nr_initsegs - so the detector says both
    there, the gated update runs, and a detector's record that did not survive a push would show in the rows."""
    import numpy as np
    from oracle.oracle import Oracle
    from tests.test_ss_big import the_list
    cfg = TAKEN[name] + (["-nr_initsegs", str(init)] if init != 10 else [])
    assert _check(cfg, BOTH) == (ceng.CTU_OK, "", 0)
    w, s = (3072, 960) if "48000" in cfg else (1103, 441)
    x = the_list(cfg)[1][:w + (frames - 1) * s + s // 2].copy()
    burg = Oracle(cfg).process(x)
    assert burg.shape[0] == frames
    for byte in (0, 1):
        f = tmp_path / ("dec%d.bin" % byte)
        f.write_bytes(bytes([byte] * frames))
        at = cfg.index("-vad") + 1
        forced = Oracle(cfg[:at] + ["file=%s" % f] + cfg[at + 1:]).process(x)
        assert forced.shape == burg.shape
        assert not np.array_equal(forced[init:], burg[init:]), (name, byte)


@pytest.mark.parametrize("cfg, word", [
    (["-format_in", "raw", "-format_out", "htk"] + K1024, "hwss / fwss / 2fwss outside the detector paths"),
    (TAKEN["fwss_44k"] + ["-fea_ncepcoefs", "33", "-fea_kind", "logspec"], "hwss / fwss / 2fwss outside the detector paths"),
    (TAKEN["fwss_44k"] + ["-fea_kind", "trapdct,101,16"], "hwss / fwss / 2fwss outside the detector paths"),
    (TAKEN["fwss_44k"] + ["-nr_when", "afterFB"], "hwss / fwss / 2fwss outside the detector paths"),
    (TAKEN["fwss_44k"] + ["-vad_out_mode", "vad"], "hwss / fwss / 2fwss outside the detector paths"),
], ids=["K1024", "ncep33", "trapdct", "afterFB", "vad_module"])
def test_what_the_engine_refuses_keeps_the_engine_s_words(cfg, word):
    got = _check(cfg, BOTH)
    assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[2] == 0 and got[1].startswith(NOT_ACCELERATED) and word in got[1], got
    for flags in (0, 1, SS, SS | 4 | 64, BOTH | 1, BOTH | 256, EVERY):
        assert _check(cfg, flags) == got, flags
    assert _check(TAKEN["fwss_44k"], BOTH)[0] == ceng.CTU_OK   # (the refusal is the option's: the configuration without it is taken)
