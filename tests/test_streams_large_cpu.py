"""Stream sets with large-transform state (CTU_STREAMS_LARGE_STATE: exten's estimate and the overlap-add's tail on 1024 .. 4096-point
frames), the parts that need no GPU: the flag's value, which configurations such a set takes, which it still refuses by name, that
without the flag the pinned refusals keep their exact words, and that on 512 points or fewer the flag changes no answer.

The flag keeps nothing of its own - it says how far the noise state and the signal state reach - so it is a flag beside one of them
only: alone, or beside the row and detector flags, 64 is answered as it always was, as an unknown flag (tests/test_host_tables.py pins
that answer for 64 alone)."""
import ctypes
import itertools

import pytest

import ctucopy_amd
from ctucopy_amd import streams_config_check
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from tests.util import C2, C3, C4, C4_NOVAD

LARGE = ceng.STREAMS_LARGE_STATE   # (the module needs the flag: on a library without it nothing here can be asked)
UNKNOWN = (ceng.CTU_ERR_INPUT, "ENGINE: unknown stream set flags")
REFUSED = "ENGINE: configuration cannot be streamed: "
EXTEN = ["-nr_mode", "exten"]
MFCC_44K = "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97".split()
MFCC_48K = "-fs 48000 -format_in raw -format_out htk -preset mfcc -preem 0.97".split()
FEATURES = {"1024": C2 + EXTEN + ["-w", "40"], "2048": MFCC_44K + EXTEN, "4096": MFCC_48K + ["-w", "64", "-s", "16"] + EXTEN}
# the speech configurations of tests/test_gpu_parity.py::test_enhancement_output_above_512_points, plain and behind exten
SPEECH_PLAIN = {"1024": "-fs 16000 -format_in raw -format_out raw -w 40 -s 20".split(),
                "2048": "-fs 44100 -format_in raw -format_out raw -w 24 -s 12.5".split(),
                "4096": "-fs 48000 -format_in raw -format_out raw -w 64 -s 16".split()}
SPEECH_EXTEN = {"1024": SPEECH_PLAIN["1024"] + EXTEN + ["-nr_a", "2"], "2048": SPEECH_PLAIN["2048"] + EXTEN,
                "2048_odd_window": "-fs 44100 -format_in raw -format_out raw -w 25 -s 10 -nr_mode exten".split()}
# what the parent commit answers, written out
WORDS_EXTEN_1024 = REFUSED + ("-nr_mode exten on 1024-point frames (-w: the noise estimate of the large transforms lives in their own kernels, "
                              "a stream set carries the one of the 256- and 512-point front end)")
WORDS_SPEECH = REFUSED + ("-format_out raw | wave on %d-point frames (-w: a stream set carries the overlap-add behind the 256- and 512-point "
                          "front end; the large transforms' synthesis is not streamed)")


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def _check(cfg, flags):
    L = ctucopy_amd.load_library()
    n, arr = ceng._argv(cfg)
    buf = ctypes.create_string_buffer(1024)
    halo = ctypes.c_int32(-1)
    rc = L.ctu_streams_config_check_ex(n, arr, flags, buf, len(buf), ctypes.byref(halo))
    return int(rc), buf.value.decode(), int(halo.value)


def test_the_flag_is_64_a_bit_of_its_own_and_2_and_16_stay_no_flags():
    assert ceng.STREAMS_LARGE_STATE == 64 and 64 & 63 == 0
    assert (ceng.STREAMS_ROW_STATE, ceng.STREAMS_NR_STATE, ceng.STREAMS_VAD_STATE, ceng.STREAMS_SIGNAL_STATE) == (1, 4, 8, 32)
    for cfg in (C2, FEATURES["1024"], SPEECH_PLAIN["2048"]):
        for bad in (2, 16, 2 | LARGE, 16 | LARGE, 2 | 16 | LARGE, 128, 128 | LARGE):
            rc, why, _ = _check(cfg, bad)
            assert rc == ceng.CTU_ERR_INPUT and "unknown stream set flags" in why, (cfg, bad)
        for alone in (LARGE, LARGE | 1, LARGE | 8, LARGE | 1 | 8):   # no state the flag could extend: the answer 64 always had
            assert _check(cfg, alone)[:2] == UNKNOWN, (cfg, alone)
        for beside in (LARGE | 4, LARGE | 32, LARGE | 4 | 32, LARGE | 1 | 4 | 8 | 32):
            assert "unknown stream set flags" not in _check(cfg, beside)[1], (cfg, beside)


@pytest.mark.parametrize("name", list(FEATURES))
def test_exten_on_the_spectrum_is_taken_at_1024_to_4096_points(name):
    cfg = FEATURES[name]
    assert streams_config_check(cfg, nr_state=True, large_state=True) == (ceng.CTU_OK, "")
    assert streams_config_check(cfg, row_state=True, nr_state=True, large_state=True) == (ceng.CTU_OK, "", 0)
    # beside the signal state alone no estimate is kept: exten's words on any set; alone the flag is none
    got = streams_config_check(cfg, signal_state=True, large_state=True)
    assert got == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-nr_mode exten (the noise estimate runs from frame to frame of a file)")
    assert streams_config_check(cfg, large_state=True) == UNKNOWN


@pytest.mark.parametrize("extra", [["-fea_E", "on"], ["-nr_a", "2", "-nr_p", "0.9", "-fea_kind", "logspec"], ["-fea_kind", "lpc"]], ids=["E", "logspec", "lpc"])
def test_the_feature_tails_behind_it_are_taken(extra):
    for name in ("1024", "2048"):
        assert streams_config_check(FEATURES[name] + extra, nr_state=True, large_state=True) == (ceng.CTU_OK, "")


def test_with_row_state_as_well_the_delta_chain_behind_exten_is_taken():
    cfg = FEATURES["1024"] + ["-fea_delta", "d_a"]
    assert streams_config_check(cfg, row_state=True, nr_state=True, large_state=True) == (ceng.CTU_OK, "", 4)
    rc, why = streams_config_check(cfg, nr_state=True, large_state=True)
    assert rc == ceng.CTU_ERR_UNSUPPORTED and why.startswith(REFUSED) and "-fea_delta" in why


@pytest.mark.parametrize("name", list(SPEECH_PLAIN))
def test_plain_speech_output_is_taken(name):
    cfg = SPEECH_PLAIN[name]
    assert streams_config_check(cfg, signal_state=True, large_state=True) == (ceng.CTU_OK, "")
    assert streams_config_check(cfg, nr_state=True, signal_state=True, large_state=True) == (ceng.CTU_OK, "")
    assert streams_config_check(cfg, row_state=True, vad_state=True, signal_state=True, large_state=True) == (ceng.CTU_OK, "", 0)
    # beside the noise state alone no tail is kept: speech output's words on any set; alone the flag is none
    assert streams_config_check(cfg, nr_state=True, large_state=True) == streams_config_check(cfg)
    assert streams_config_check(cfg, large_state=True) == UNKNOWN


@pytest.mark.parametrize("name", list(SPEECH_EXTEN))
def test_speech_output_behind_exten_is_taken_with_the_noise_state_as_well(name):
    cfg = SPEECH_EXTEN[name]
    assert streams_config_check(cfg, nr_state=True, signal_state=True, large_state=True) == (ceng.CTU_OK, "")
    got = streams_config_check(cfg, signal_state=True, large_state=True)
    assert got == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-nr_mode exten (the noise estimate runs from frame to frame of a file)")


VAD = ["-vad_out_mode", "vad", "-vad_cri_mode", "energy", "-vad_thr_mode", "adapt"]


@pytest.mark.parametrize("cfg, words", [
    (C2 + EXTEN + ["-nr_when", "afterFB"], ["-nr_when afterFB"]),
    (MFCC_44K + ["-nr_mode", "fwss", "-vad", "burg"], ["-nr_mode fwss"]),
    ("-fs 44100 -format_in raw -format_out raw -w 24 -s 12.5 -nr_mode fwss -vad burg".split(), ["-nr_mode fwss"]),
    (FEATURES["2048"] + ["-remove_dc1", "on"], ["-remove_dc1"]),
    (SPEECH_EXTEN["2048"] + ["-remove_dc1", "on"], ["-remove_dc1"]),
    (C2 + ["-w", "40"] + VAD, ["the VAD module"]),
    (MFCC_44K + VAD, ["the VAD module"]),
    (MFCC_44K + VAD + EXTEN, ["the VAD module"]),
], ids=["afterFB", "fwss", "fwss_speech", "remove_dc1", "remove_dc1_speech", "vad_1024", "vad_2048", "vad_2048_exten"])
def test_what_is_still_refused_by_name_whatever_the_flags(cfg, words):
    speech = cfg[cfg.index("-format_out") + 1] == "raw"   # (without the signal state speech output is refused as such, ahead of the rest)
    for row, vad, sig_ in itertools.product((False, True), (False, True), (True,) if speech else (False, True)):
        got = streams_config_check(cfg, row_state=row, nr_state=True, vad_state=vad, signal_state=sig_, large_state=True)
        assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[1].startswith(REFUSED), got
        for w in words:
            assert w in got[1], got
    rc, why, _ = _check(cfg, 1 | 4 | 8 | LARGE)
    if "the VAD module" in words:   # with detector state: refused by size, in the words the parent has for it
        assert why == REFUSED + "the VAD module on 1024-point and larger frames (-w: a stream set carries the detector behind the 256- and 512-point front end)"


def test_exten_behind_the_filter_bank_at_the_large_sizes_stays_the_engines_refusal():
    """ctu_engine_create takes exten at 1024 .. 4096 points on the spectrum only: there is no engine to make a set on, whatever the flags."""
    for name in ("1024", "2048"):
        for flags in (4 | LARGE, 1 | 4 | LARGE, 1 | 4 | 8 | 32 | LARGE):
            rc, why, _ = _check(FEATURES[name] + ["-nr_when", "afterFB"], flags)
            assert rc == ceng.CTU_ERR_UNSUPPORTED and why.startswith("ENGINE: configuration not on the accelerated path: "), (name, flags, why)


def test_without_the_flag_the_pinned_refusals_keep_their_exact_words():
    for flags in (4, 1 | 4, 4 | 8, 4 | 32):
        rc, why, halo = _check(FEATURES["1024"], flags)
        assert (rc, why, halo) == (ceng.CTU_ERR_UNSUPPORTED, WORDS_EXTEN_1024, 0), flags
    for cfg, points in ((SPEECH_PLAIN["1024"], 1024), (SPEECH_PLAIN["2048"], 2048), (SPEECH_EXTEN["2048"], 2048)):
        for flags in (4 | 32, 1 | 4 | 32, 4 | 8 | 32):
            rc, why, halo = _check(cfg, flags)
            assert (rc, why, halo) == (ceng.CTU_ERR_UNSUPPORTED, WORDS_SPEECH % points, 0), (cfg, flags)
    assert _check(SPEECH_PLAIN["1024"], 32)[1] == WORDS_SPEECH % 1024


SIG16 = "-fs 16000 -format_in raw -format_out raw".split()
PLAIN = ["-nr_mode", "none", "-fea_kind", "none", "-fb_definition", "none"]
SMALL = {
    "mfcc": C2, "plp": C3, "mfcc_exten": C2 + EXTEN, "c4_novad": C4_NOVAD, "c4_vad": C4, "d_a": C2 + ["-fea_delta", "d_a"],
    "afterFB": C2 + EXTEN + ["-nr_when", "afterFB"], "fwss": C2 + ["-nr_mode", "fwss", "-vad", "burg"],
    "speech_exten": SIG16 + ["-preset", "exten"], "speech_plain": SIG16 + PLAIN + ["-w", "25", "-s", "10", "-preem", "0.97"],
    "speech_dc1": SIG16 + PLAIN + ["-remove_dc1", "on"], "bad_option": "-fs 16000 -bogus 1".split(),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_on_512_points_or_fewer_the_flag_changes_no_answer(name):
    cfg = SMALL[name]
    for flags in sorted({a | b | c | d for a, b, c, d in itertools.product((0, 1), (0, 4), (0, 8), (0, 32))}):
        if flags & (4 | 32):
            assert _check(cfg, flags | LARGE) == _check(cfg, flags), flags
        else:   # no state the flag could extend: what any unknown flag is answered
            assert _check(cfg, flags | LARGE) == _check(cfg, flags | 2), flags


def test_without_exten_or_speech_output_the_flag_changes_nothing_at_the_large_sizes_either():
    for cfg in (C2 + ["-w", "40"], MFCC_44K, MFCC_44K + ["-fea_delta", "d_a"], MFCC_44K + ["-fea_kind", "trapdct"]):
        for flags in (4, 1 | 4, 1 | 4 | 8, 32, 4 | 32):
            assert _check(cfg, flags | LARGE) == _check(cfg, flags), (cfg, flags)
