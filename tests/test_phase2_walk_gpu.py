"""The straight-line filter-bank walk of the preset banks computes the generic walk's rows byte for byte.

Both walks read the same tables with the same lane mapping and add in the same order, so there is no tolerance: the
rows of C2, C3 and C5 on the miniature synthetic set must be equal as bit patterns with the specialised walk and with
the generic one forced (CTU_PHASE2_GENERIC=1 is read when an engine is created).
"""
import numpy as np
import pytest

from tests.util import C2, C3, C5, sig, synth_utt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def _utts(short):
    from ctucopy_amd import synth
    # the 16 miniatures, plus lengths around the 8-frame step and the 64-frame tile
    return ([synth.utterance_c(synth.SET_SPEECH, i, True) for i in range(16)] + [sig("CS0")[:40000]] +
            [synth_utt(70 + f, 240 + 160 * f + 3) for f in short])


@pytest.mark.parametrize("name,cfg,index", [("C2", C2, 0), ("C3", C3, 1), ("C5", C5, 2)])
def test_specialised_walk_rows_equal_generic_walk_rows(Engine, monkeypatch, name, cfg, index):
    # (the TRAP chain of C5 is undefined on fewer than 51 frames: the engine refuses such a list, as the reference does)
    utts = _utts((51, 57, 63, 64, 65) if name == "C5" else (1, 7, 8, 9, 63, 64, 65))
    monkeypatch.delenv("CTU_PHASE2_GENERIC", raising=False)
    spec = Engine(cfg)
    monkeypatch.setenv("CTU_PHASE2_GENERIC", "1")
    gen = Engine(cfg)
    assert gen.kernel_name() == spec.kernel_name()  # the walk does not show in the name that keys the profiles
    rows_s, rows_g = spec.extract(utts), gen.extract(utts)
    # what the launches really ran: the straight-line kernel of this preset, and the generic one
    assert spec.phase2_walk() == index
    assert gen.phase2_walk() == -1
    nrows = 0
    for a, b in zip(rows_s, rows_g):
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.isfinite(a).all()
        nrows += a.shape[0]
    assert nrows > 1000


def test_other_banks_and_instantiations_run_the_generic_walk(Engine, monkeypatch):
    monkeypatch.delenv("CTU_PHASE2_GENERIC", raising=False)
    utts = _utts((51, 64))
    for cfg in (C2 + ["-w", "24"],                                    # another frame shape
                "-fs 8000 -format_in raw -format_out htk -preset mfcc".split(),   # another bank, the 256-point kernel
                C2 + ["-fb_definition", "23filters"],                 # C5's bank in front of the DCT: no such instantiation is compiled
                C2 + ["-nr_mode", "exten"]):                          # the headline's bank on the exten instantiation
        eng = Engine(cfg)
        eng.extract(utts)
        assert eng.phase2_walk() == -1, cfg
