"""Stream sets with noise state (CTU_STREAMS_NR_STATE), the parts that need no GPU: which configurations with -nr_mode exten such a set
takes, which it still refuses and with what words, and that the flag changes no other answer."""
import pytest

from ctucopy_amd import streams_config_check
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from tests.util import C2, C3, C4, C4_NOVAD

EXTEN = ["-nr_mode", "exten"]
REFUSED = "ENGINE: configuration cannot be streamed: "


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def test_the_flag_is_a_bit_of_its_own_and_combines_with_row_state():
    assert ceng.STREAMS_NR_STATE not in (0, ceng.STREAMS_ROW_STATE) and ceng.STREAMS_NR_STATE & ceng.STREAMS_ROW_STATE == 0
    assert ceng.STREAMS_NR_STATE & (ceng.STREAMS_NR_STATE - 1) == 0


@pytest.mark.parametrize("cfg", [C2 + EXTEN, C4_NOVAD, C3 + EXTEN], ids=["mfcc_exten", "c4_novad", "plp_exten"])
def test_exten_on_the_spectrum_is_taken(cfg):
    assert streams_config_check(cfg, nr_state=True) == (ceng.CTU_OK, "")
    assert streams_config_check(cfg, row_state=True, nr_state=True) == (ceng.CTU_OK, "", 0)


def test_with_row_state_as_well_the_chains_behind_exten_are_taken():
    cfg = C2 + EXTEN + ["-fea_delta", "d_a", "-fea_Z_exp", "500"]
    assert streams_config_check(cfg, row_state=True, nr_state=True) == (ceng.CTU_OK, "", 4)
    rc, why = streams_config_check(cfg, nr_state=True)   # the noise state alone does not hold rows back
    assert rc == ceng.CTU_ERR_UNSUPPORTED and why.startswith(REFUSED) and "-fea_delta" in why


@pytest.mark.parametrize("cfg, words", [
    (C2 + EXTEN + ["-nr_when", "afterFB"], ["-nr_when afterFB"]),
    (C2 + EXTEN + ["-w", "40"], ["-nr_mode exten", "1024-point"]),
    (C2 + ["-nr_mode", "fwss", "-vad", "burg"], ["-nr_mode fwss"]),
    (C4, ["VAD module"]),
    (C2 + ["-remove_dc1", "on"] + EXTEN, ["-remove_dc1"]),
    ("-fs 16000 -format_in raw -format_out raw -preset exten".split(), ["-format_out raw"]),
], ids=["afterFB", "1024_points", "fwss", "vad_module", "remove_dc1", "speech_output"])
def test_what_a_set_with_noise_state_still_refuses_by_name(cfg, words):
    for row_state in (False, True):
        got = streams_config_check(cfg, row_state=row_state, nr_state=True)
        assert got[0] == ceng.CTU_ERR_UNSUPPORTED and got[1].startswith(REFUSED), got
        for w in words:
            assert w in got[1], got
        if row_state:
            assert got[2] == 0


def test_without_the_flag_exten_is_refused_with_the_words_it_had():
    for kw in ({}, {"row_state": True}):
        got = streams_config_check(C2 + EXTEN, **kw)
        assert got[0] == ceng.CTU_ERR_UNSUPPORTED
        assert got[1] == REFUSED + "-nr_mode exten (the noise estimate runs from frame to frame of a file)"


@pytest.mark.parametrize("cfg", [C2, C3, C2 + ["-fea_delta", "d_a"], C2 + ["-fea_Z_exp", "500"], C2 + ["-w", "40"],
                                 C2 + ["-remove_dc1", "on"], "-fs 16000 -bogus 1".split()],
                         ids=["mfcc", "plp", "d_a", "Zexp", "1024", "remove_dc1", "bad_option"])
def test_without_noise_reduction_the_flag_changes_no_answer(cfg):
    assert streams_config_check(cfg, nr_state=True) == streams_config_check(cfg)
    assert streams_config_check(cfg, row_state=True, nr_state=True) == streams_config_check(cfg, row_state=True)
