"""Stream sets with subtraction state (CTU_STREAMS_SS_STATE: what -nr_mode hwss | fwss | 2fwss carry along a file, kept per stream), the
parts that need no GPU: the flag's value, which configurations such a set takes and with which halo, what it refuses by name, that
what the engine itself refuses keeps the engine's words, that without the flag every answer keeps the words it had, and that beside a
configuration without one of the three modes the flag changes no answer.

The answers "without the flag" are written out here from the words tests/test_streams_cpu.py, tests/test_streams_rows_cpu.py and
tests/golden/host_tables.json pin, not taken from the code under test."""
import ctypes
import itertools

import pytest

import ctucopy_amd
from ctucopy_amd import streams_config_check
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from tests.util import C2, C5

SS = 1024
UNKNOWN = (ceng.CTU_ERR_INPUT, "ENGINE: unknown stream set flags")
REFUSED = "ENGINE: configuration cannot be streamed: "
NOT_ACCELERATED = "ENGINE: configuration not on the accelerated path: "
SS8 = "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97 -vad burg".split()   # tests/test_gpu_parity.py, rows a10 / N4
C2B = C2 + ["-vad", "burg"]
M44B = "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97 -vad burg".split()
FWSS, FWSS2, HWSS = ["-nr_mode", "fwss"], ["-nr_mode", "2fwss"], ["-nr_mode", "hwss", "-fea_kind", "spec"]
D_A_Z = ["-fea_delta", "d_a", "-fea_Z_exp", "0.95"]
SIG_FWSS = "-fs 16000 -format_in raw -format_out raw -w 25 -s 12.5 -nr_mode fwss -vad burg".split()   # tests/util.py: sig_fwss
PLP = ["-fb_eqld", "on", "-fb_inld", "on", "-fea_kind", "lpc", "-fea_lporder", "12"]


def _words(mode):
    return REFUSED + "-nr_mode %s (the noise estimate runs from frame to frame of a file)" % mode   # today's sentence, flags 0


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


def test_the_flag_is_1024_and_2_16_128_and_512_stay_no_flags():
    assert ceng.STREAMS_SS_STATE == SS == 1024
    assert (ceng.STREAMS_ROW_STATE, ceng.STREAMS_NR_STATE, ceng.STREAMS_VAD_STATE, ceng.STREAMS_SIGNAL_STATE, ceng.STREAMS_LARGE_STATE,
            ceng.STREAMS_TRAP_STATE) == (1, 4, 8, 32, 64, 256)
    for cfg in (C2, SS8 + FWSS, C2B + FWSS2):
        assert "unknown stream set flags" not in _check(cfg, SS)[1], cfg
        assert "unknown stream set flags" not in _check(cfg, SS | 1)[1], cfg
        for bad in (2, 16, 128, 512):
            assert _check(cfg, bad)[:2] == UNKNOWN, (cfg, bad)
            assert _check(cfg, bad | SS)[:2] == UNKNOWN, (cfg, bad)
        # 64 is a flag only beside the noise state or the signal state: the subtraction state is neither
        for alone in (64 | SS, 64 | SS | 1):
            assert _check(cfg, alone)[:2] == UNKNOWN, (cfg, alone)


def test_the_binding_carries_the_flag():
    assert ceng._stream_flags(True, True, True, True, True, True) == 1 | 4 | 8 | 32 | 64 | 256   # the six-argument call is what it was
    assert ceng._stream_flags(False, False, False, ss_state=True) == 1024
    assert ceng._stream_flags(True, True, True, True, True, True, True) == 1 | 4 | 8 | 32 | 64 | 256 | 1024
    assert streams_config_check(SS8 + FWSS, ss_state=True) == (ceng.CTU_OK, "")
    assert streams_config_check(SS8 + FWSS2 + D_A_Z, ss_state=True, row_state=True) == (ceng.CTU_OK, "", 4)
    assert streams_config_check(SS8 + FWSS) == (ceng.CTU_ERR_UNSUPPORTED, _words("fwss"))
    assert streams_config_check(C2, ss_state=True) == (ceng.CTU_OK, "")


@pytest.mark.parametrize("cfg", [
    SS8 + FWSS, SS8 + FWSS2, SS8 + HWSS, C2B + FWSS,
    SS8 + FWSS + ["-fea_E", "on"], C2B + FWSS + ["-fea_E", "on"],
    SS8 + FWSS + PLP, C2B + FWSS + ["-fea_kind", "lpc", "-fea_lporder", "10"],
    SS8 + FWSS + ["-w", "20", "-s", "10"], C2B + FWSS + ["-w", "20", "-s", "10"],
    SS8 + FWSS + ["-fea_ncepcoefs", "3"], SS8 + FWSS + ["-fea_kind", "spec", "-fea_ncepcoefs", "3"],
    C2B + FWSS + ["-fea_kind", "logspec", "-fea_ncepcoefs", "16"], SS8 + FWSS2 + ["-fea_kind", "spec", "-fea_ncepcoefs", "16"],
], ids=["fwss", "2fwss", "hwss_spec", "c2_fwss", "E", "c2_E", "plp", "c2_lpc10", "w20", "c2_w20", "ncep3", "spec_ncep3", "c2_logspec_ncep16",
        "2fwss_spec_ncep16"])
def test_the_modes_are_taken_on_the_feature_path_with_no_halo(cfg):
    assert _check(cfg, SS) == (ceng.CTU_OK, "", 0)
    # ... whatever other flags come with it (none of them bears on a configuration without exten, the VAD module, speech output, trapdct)
    assert _check(cfg, SS | 1 | 4 | 8 | 32 | 256) == (ceng.CTU_OK, "", 0)
    assert _check(cfg, 0) == (ceng.CTU_ERR_UNSUPPORTED, _words(_mode(cfg)), 0)


def test_the_chains_behind_them_need_the_row_state_as_ever():
    cfg = SS8 + FWSS2 + D_A_Z
    assert _check(cfg, SS | 1) == (ceng.CTU_OK, "", 4)   # the chain's halo
    assert _check(cfg, SS) == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-fea_delta (the delta chain spans the frames of its windows)", 0)
    # (-fea_Z_exp is a time constant in ms: 0.95 is below two hops and switches CMS off, src/io/opts.cc; 500 is a running mean)
    assert _check(SS8 + FWSS + ["-fea_Z_exp", "500"], SS) == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-fea_Z_exp (CMS: the running mean runs along the file)", 0)
    assert _check(SS8 + FWSS + ["-fea_Z_exp", "500"], SS | 1) == (ceng.CTU_OK, "", 0)
    assert _check(C2B + FWSS + ["-fb_inld", "on", "-fea_trap", "5"], SS | 1) == (ceng.CTU_OK, "", 2)   # stacking of five frames: two either side
    assert _check(cfg, 1) == (ceng.CTU_ERR_UNSUPPORTED, _words("2fwss"), 0)


@pytest.mark.parametrize("cfg, flags, word", [
    (SS8[:-2] + ["-vad", "file=dec.bin"] + FWSS, SS, "-vad file=... with -nr_mode fwss"),
    (SIG_FWSS, SS, "-nr_mode fwss with -format_out raw | wave"),
    (SIG_FWSS, SS | 32, "-nr_mode fwss with -format_out raw | wave"),
    (M44B + ["-nr_mode", "hwss"], SS, "-nr_mode hwss on 2048-point frames"),
    (M44B + FWSS2, SS | 4 | 64, "-nr_mode 2fwss on 2048-point frames"),
    (C2 + ["-remove_dc1", "on"], SS, "-remove_dc1"),
    (SS8 + FWSS + ["-s", "30"], SS, "-s above -w"),
], ids=["vad_file", "speech_output", "speech_output_signal_flag", "hwss_2048", "2fwss_2048_large", "remove_dc1", "s_above_w"])
def test_what_is_refused_with_the_flag_is_refused_by_name(cfg, flags, word):
    rc, why, halo = _check(cfg, flags)
    assert rc == ceng.CTU_ERR_UNSUPPORTED and halo == 0 and why.startswith(REFUSED) and word in why, why
    assert _check(cfg, flags & ~SS)[0] == ceng.CTU_ERR_UNSUPPORTED


@pytest.mark.parametrize("cfg, word", [
    (C2B + FWSS + ["-w", "30"], "hwss / fwss / 2fwss outside the detector paths"),
    (SS8 + FWSS + ["-fea_kind", "spec", "-fea_ncepcoefs", "17"], "hwss / fwss / 2fwss outside the detector paths"),
    (SS8 + FWSS + ["-stat_cmvn", "s.txt"], "hwss / fwss / 2fwss outside the detector paths"),
    (SS8 + ["-nr_mode", "hwss", "-nr_when", "afterFB"], "hwss / fwss / 2fwss outside the detector paths"),
    (SS8 + FWSS + ["-remove_dc1", "on"], "no -remove_dc1"),
    (C5 + ["-vad", "burg"] + FWSS, "hwss / fwss / 2fwss"),
], ids=["w30_16k", "17_coefficients", "cmvn", "afterFB", "remove_dc1", "trapdct"])
def test_what_the_engine_refuses_keeps_the_engine_s_words(cfg, word):
    got = _check(cfg, SS)
    assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[2] == 0 and got[1].startswith(NOT_ACCELERATED) and word in got[1], got
    for flags in (0, 1, SS | 1, SS | 4 | 8 | 32):
        assert _check(cfg, flags) == got, flags


@pytest.mark.parametrize("cfg", [SS8 + FWSS, SS8 + FWSS2, SS8 + HWSS, C2B + FWSS, C2B + FWSS2 + D_A_Z, SS8 + FWSS + PLP, M44B + ["-nr_mode", "hwss"]],
                         ids=["fwss", "2fwss", "hwss_spec", "c2_fwss", "c2_2fwss_d_a_Z", "plp", "hwss_2048"])
def test_without_the_flag_every_answer_is_the_sentence_it_was(cfg):
    want = (ceng.CTU_ERR_UNSUPPORTED, _words(_mode(cfg)), 0)
    for flags in _subsets([1, 4, 8, 32]):
        assert _check(cfg, flags) == want, flags
        assert _check(cfg, flags | 256) == want, flags
        if flags & (4 | 32):
            assert _check(cfg, flags | 64) == want, flags
            assert _check(cfg, flags | 64 | 256) == want, flags


@pytest.mark.parametrize("cfg", [C2, C2 + ["-nr_mode", "exten"], C5], ids=["C2", "C2_exten", "C5"])
def test_beside_another_configuration_the_flag_changes_no_answer(cfg):
    for flags in _subsets([1, 4, 8, 32, 256]) + [64 | 4, 64 | 32, 64 | 4 | 32 | 1 | 8 | 256]:
        assert _check(cfg, flags | SS) == _check(cfg, flags), flags
    assert _check(C2 + ["-nr_mode", "exten"], SS) == (ceng.CTU_ERR_UNSUPPORTED, REFUSED + "-nr_mode exten (the noise estimate runs from frame to frame of a file)", 0)
    assert _check(C2 + ["-nr_mode", "exten"], SS | 4) == (ceng.CTU_OK, "", 0)
    assert _check(C5, SS | 256) == (ceng.CTU_OK, "", 50)
