"""Stage 2 of the packed DUAL front end on column pairs (frontend_kernel.h, the DUAL block; maps: paircol_map.h).

Two things are held:
  every bin, seen directly   band spectra (-fea_kind spec on the plain chain) of inputs that put their energy into one bin - the two
      self-mirrored columns of lane p = 0 (bins 0, 8, 16, 128, 248, 256 ...), the general pairs and both specials - against the
      oracle, with the comparison and tolerance tests/test_gpu_parity.py applies to that kind;
  step and tile edges        the rows of C2, C3 and C5 on utterances around the 8-frame step and the 64-frame tile, as bit patterns
      against tests/golden/paircol_parent_rows.npz.  That file holds this project's own rows as a library built from the PARENT
      commit of the change wrote them on the GPU (tests/golden/make_paircol_parent_rows.py; its `how` entry says so): the new lane map
      moves every operand and changes no operation, so there is no tolerance.  (The utterance that starts with silence has rows that are
      not finite - a frame of zeros has no logarithm; they are compared as patterns like the rest.)
Each configuration is first shown to run a 13-row MODE 0 plain or plain + inld instantiation - the ones whose phase 1 is that block."""
import os

import numpy as np
import pytest

from ctucopy_amd import config_table
from tests.test_gpu_parity import _check
from tests.util import C2, C3, C5, GOLDEN, square_fs, synth_utt

pytestmark = pytest.mark.gpu

SPEC = C2 + ["-fea_kind", "spec"]
FIELDS = ("nz", "feat", "mode", "vx", "nc", "gen", "lpo", "md", "vf", "ss", "sy", "walk")
WINDOW, SHIFT = 400, 160
TONE_BINS = (0, 1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 247, 248, 249, 255, 256)
# The parity bound (1e-4 element-wise) holds where the fp32 transform's noise floor, about 1e-7 of the frame's largest bin, stays below 1e-4
# of the smallest band (tests/test_gpu_parity.py: _assert_rows).  A tone of amplitude A puts about 108 A (half the Hamming window's sum)
# into one bin, while the bands far from it hold nothing but the tone's rounding to int16: +-0.5 LSB, uniform, about 0.29 sqrt(sum w^2) = 3
# per bin.  The floor reaches 1e-4 of those bands at 108 A x 1e-7 x (a few) = 3e-4, A of a few tens; louder tones only measure the
# format.  A = 8 leaves a factor of two or more, and the tone's own bands still stand 50 dB above the rest.
AMPLITUDE = 8


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def runs_the_packed_dual_block(cfg):
    """fe_dual (layout_constants.h) with 13 rows: what ctu_engine_create selects for cfg, from the host side."""
    k = dict(zip(FIELDS, (int(x) for x in config_table(cfg, "frontend"))))
    return k["nz"] == 13 and k["mode"] == 0 and k["gen"] in (0, 1) and not (k["vx"] or k["vf"] or k["ss"] or k["sy"])


def frames(n):
    return WINDOW + SHIFT * (n - 1)


def tone(b, nframes=3):
    """A cosine centred on bin b of the 512-point transform; b = 0 is a constant, b = 256 alternates +-A."""
    n = np.arange(frames(nframes))
    return np.round(AMPLITUDE * np.cos(2 * np.pi * b * n / 512)).astype(np.int16)


def impulse(at, value, nframes=3):
    """`value` at sample `at` of the second frame, zeros elsewhere."""
    x = np.zeros(frames(nframes), np.int16)
    x[SHIFT + at] = value
    return x


def direct_inputs():
    utts = [tone(b, 2 + (i % 2)) for i, b in enumerate(TONE_BINS)]
    utts += [impulse(at, v) for at in (0, 1, 399) for v in (1, 32767)]
    utts += [np.zeros(frames(2), np.int16), square_fs(frames(3))]
    return utts


def test_every_bin_against_the_oracle(Engine):
    assert runs_the_packed_dual_block(SPEC)
    eng = Engine(SPEC)
    assert eng.kernel_name().startswith("frontend_kernel<13, BANDS, MODE 0, plain")
    utts = direct_inputs()
    worst = _check(Engine, SPEC, utts)
    print("spec rows of %d direct inputs: worst element-wise error %.3g" % (len(utts), worst))


# ---- step and tile edges, bit for bit against the parent's rows
EDGE_FRAMES = {"C2": (1, 3, 4, 5, 7, 8, 9, 63, 64, 65), "C3": (1, 3, 4, 5, 7, 8, 9, 63, 64, 65), "C5": (51, 57, 63, 64, 65)}
EDGE_CFG = {"C2": C2, "C3": C3, "C5": C5}
EDGE_KERNEL = {"C2": "frontend_kernel<13, DCTC, MODE 0, plain, MD>", "C3": "frontend_kernel<13, LP, MODE 0, inld, MD>",
               "C5": "frontend_kernel<13, BANDS, MODE 0, plain>"}


def edge_utts(name):
    """(the TRAP chain of C5 is undefined on fewer than 51 frames: the engine refuses such a list, as the reference does)"""
    utts = [synth_utt(70 + f, 240 + 160 * f + 3) for f in EDGE_FRAMES[name]]
    lead = synth_utt(69, 240 + 160 * (52 if name == "C5" else 12) + 3)
    lead[:1000] = 0  # starts with silence: whole frames of zeros, then one that is partly zeros
    return utts + [lead]


@pytest.fixture(scope="module")
def parent_rows():
    z = np.load(os.path.join(GOLDEN, "paircol_parent_rows.npz"))
    assert "parent commit" in str(z["how"])
    return z


@pytest.mark.parametrize("name", ["C2", "C3", "C5"])
def test_step_and_tile_edges_are_the_parents_rows_bit_for_bit(Engine, parent_rows, name):
    cfg = EDGE_CFG[name]
    assert runs_the_packed_dual_block(cfg)
    eng = Engine(cfg)
    assert eng.kernel_name() == EDGE_KERNEL[name]
    utts = edge_utts(name)
    rows = eng.extract(utts)
    assert [r.shape[0] for r in rows[:-1]] == list(EDGE_FRAMES[name])
    for i, r in enumerate(rows):
        want = parent_rows["%s_%d" % (name, i)]
        assert r.dtype == np.float32 and want.dtype == np.uint32 and r.shape == want.shape
        diff = np.flatnonzero(r.view(np.uint32) != want)
        assert diff.size == 0, "%s utterance %d: %d of %d words differ, first at %d" % (name, i, diff.size, want.size, diff[0])
