"""The compiled walk signatures of phase 2 (ctucopy_amd/csrc/phase2_walks.h) against what build_phase2 lays out.

The three preset configurations that the benchmark runs must land on their straight-line walk: a change to the bank
design or to build_phase2's sort would otherwise drop them onto the generic walk without any test noticing.  Banks
and frame shapes that no signature was compiled for must report -1.  No GPU needed: the tables are host work.
"""
import pytest

from ctucopy_amd import config_table
from tests.util import C1, C2, C3, C4_NOVAD, C5

# index in phase2_walks.h, chunks per slot
PRESETS = {
    "C2": (C2, 0, [13, 6, 4, 2]),
    "C3": (C3, 1, [29, 11, 4]),
    "C5": (C5, 2, [13, 6, 3]),
}
NON_PRESETS = {
    "30filters": C1,                                     # another bank definition
    "mel20": C2 + ["-fb_definition", "20filters"],       # another number of bands
    "8kHz": C4_NOVAD,                                    # another sample rate: the 256-point kernel
    "8kHz_plp": "-fs 8000 -format_in raw -format_out htk -preset plpc".split(),
    "w24": C2 + ["-w", "24"],                            # same bank, another window length inside the 512-point kernel
    "w20": C2 + ["-w", "20"],
    "plp_w20": C3 + ["-w", "20"],
}


@pytest.mark.parametrize("name", sorted(PRESETS))
def test_preset_banks_match_their_compiled_signature(name):
    cfg, index, chunks = PRESETS[name]
    walk = config_table(cfg, "phase2_walk")
    assert [int(x) for x in walk[:-1]] == chunks
    assert int(walk[-1]) == index


def test_match_is_by_bank_and_frame_shape():
    # "phase2_walk" compares chunk counts and frame shape only: C5's bank in front of the DCT, or the headline's bank with exten,
    # match an entry although the instantiation they run on has no straight-line form (such engines launch the generic walk and
    # ctu_engine_phase2_walk says so: tests/test_phase2_walk_gpu.py)
    assert int(config_table(C2 + ["-fb_definition", "23filters"], "phase2_walk")[-1]) == 2
    assert int(config_table(C2 + ["-nr_mode", "exten"], "phase2_walk")[-1]) == 0


@pytest.mark.parametrize("name", sorted(NON_PRESETS))
def test_other_banks_take_the_generic_walk(name):
    walk = config_table(NON_PRESETS[name], "phase2_walk")
    assert int(walk[-1]) == -1
    assert len(walk) >= 2 and all(x >= 1 for x in walk[:-1])


@pytest.mark.parametrize("name", sorted(PRESETS) + sorted(NON_PRESETS))
def test_walk_agrees_with_phase2_check(name):
    cfg = PRESETS[name][0] if name in PRESETS else NON_PRESETS[name]
    err, nchunks, nslots = config_table(cfg, "phase2_check")
    walk = config_table(cfg, "phase2_walk")
    assert err == 0.0
    assert len(walk) == int(nslots) + 1 and sum(walk[:-1]) == nchunks
