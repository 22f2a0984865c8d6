"""Hi-res MFCC (dctc with 25 to 64 values per frame) is on the accelerated path: a band-valued front end, then dct_wide_kernel
(ctucopy_amd/csrc/dctw_kernel.h).  Without a GPU the engine gets as far as opening the device (unsupported_reason runs before that);
the selection, the table and what stays refused are checked on the host."""
import numpy as np
import pytest

import ctucopy_amd
from ctucopy_amd import CtuError, config_dims, config_table
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.util import C2

HI = C2 + ["-fb_definition", "1-40/40filters", "-fea_ncepcoefs", "39"]
B64 = C2 + ["-fb_definition", "1-64/64filters", "-fea_ncepcoefs", "63", "-fea_E", "on"]
K8 = "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97 -fb_definition 1-40/40filters -fea_ncepcoefs 39".split()
REACH = [(HI, 40), (B64, 65), (HI + ["-fea_c0", "off"], 39), (K8, 40), (HI + ["-w", "40"], 40), (HI + ["-w", "80"], 40),
         (HI + ["-nr_mode", "exten"], 40), (HI + ["-fea_delta", "d_a"], 120),
         (C2 + ["-fea_ncepcoefs", "30"], 31), (C2 + ["-fb_definition", "1-30/30filters", "-fea_ncepcoefs", "29", "-fea_Z_exp", "500"], 30)]
FIELDS = ("nz", "feat", "mode", "vx", "nc", "gen", "lpo", "md", "vf", "ss", "sy", "walk")
BANDS, DCTC = 0, 2   # layout_constants.h: FeatMode


def ident(c):
    return " ".join(c[c.index("-preset") + 2:]) + " @" + c[1]


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def sel(cfg):
    return dict(zip(FIELDS, (int(x) for x in config_table(cfg, "frontend"))))


@pytest.mark.parametrize("cfg,width", REACH, ids=[ident(c) for c, _ in REACH])
def test_geometry_and_oracle(cfg, width):
    d = config_dims(cfg)
    assert d.row_floats == width
    assert Oracle(cfg).dims.D == width   # the checker restates the configuration with the same row


def test_htk_header_fields_of_forty_columns():
    d = config_dims(HI)
    assert (d.row_floats, d.htk_kind, d.htk_period) == (40, 8198, 100000)   # MFCC_0, 160 bytes a sample
    assert config_dims(B64).htk_kind == 8198 | 0o100                         # _E


@pytest.mark.parametrize("cfg", [c for c, _ in REACH], ids=ident)
def test_hires_configurations_reach_the_device(cfg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    Oracle(cfg)   # the checker accepts the configuration
    with pytest.raises(CtuError) as ei:
        ctucopy_amd.Engine(cfg)
    assert ei.value.code == ceng.CTU_ERR_DEVICE and "no CPU fallback" in str(ei.value), str(ei.value)


def test_the_boundary_is_24_values_per_frame():
    k23 = sel(C2 + ["-fea_ncepcoefs", "23"])
    # today's DCTC instantiation with rows of MAXC entries, as tests/golden/frontend_selection.json records it for `wide_mfcc`
    assert [k23[f] for f in FIELDS] == [13, DCTC, 0, 0, 24, 0, 0, 0, 0, 0, 0, -1]
    k24 = sel(C2 + ["-fea_ncepcoefs", "24"])
    assert k24["feat"] == BANDS and k24["nc"] == 16 and k24["gen"] == 0
    with pytest.raises(CtuError) as ei:
        ctucopy_amd.Engine(C2 + ["-fb_definition", "1-64/64filters", "-fea_ncepcoefs", "64"])
    assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and "more than 64 cepstral values" in str(ei.value), str(ei.value)


def test_the_front_end_ahead_of_the_tail_is_band_valued():
    assert sel(HI)["feat"] == BANDS and sel(HI)["gen"] == 0                      # plain
    assert sel(HI + ["-nr_mode", "exten"])["gen"] == 2                           # exten
    assert sel(B64)["gen"] == 3 and sel(B64)["feat"] == BANDS                    # -fea_E: the flags at run time
    assert sel(K8)["mode"] == 1 and sel(K8)["feat"] == BANDS
    assert [int(x) for x in config_table(HI + ["-w", "40"], "frontend")] == [0] * 11 + [-1]   # the large-FFT kernels


@pytest.mark.parametrize("extra,reason", [
    (["-fea_ncepcoefs", "64"], "more than 64 cepstral values"),
    (["-nr_mode", "fwss", "-vad", "burg"], "hwss / fwss / 2fwss with more than 24 cepstral values"),
    (["-nr_mode", "hwss", "-vad", "burg"], "hwss / fwss / 2fwss with more than 24 cepstral values"),
    (["-nr_mode", "2fwss", "-vad", "burg"], "hwss / fwss / 2fwss with more than 24 cepstral values"),
    (["-vad_out_mode", "vad", "-vad_cri_mode", "energy"], "the VAD module beside more than 24"),
    (["-vad_out_mode", "vad", "-vad_cri_mode", "cepdist", "-vad_cepdist_mode", "lpc", "-vad", "burg"], "the VAD module beside more than 24"),
    (["-vad_out_mode", "vad", "-vad_cri_mode", "cepdist", "-vad_cepdist_mode", "fea"], "the VAD module beside more than 24"),
    (["-nr_mode", "exten", "-nr_when", "afterFB"], "-nr_when afterFB with more than 24"),
    (["-fea_kind", "lpc", "-fea_lporder", "24", "-fea_ncepcoefs", "24"], "above 23"),
    (["-fea_kind", "lpa", "-fea_lporder", "24", "-fea_ncepcoefs", "24"], "above 23"),
    (["-fea_Z_exp", "500"], "more than 32 CMS columns"),
    (["-fea_trap", "on", "-d_win", "15"], "delta / stacking tile"),
])
def test_what_stays_refused_names_itself(extra, reason):
    with pytest.raises(CtuError) as ei:
        ctucopy_amd.Engine(C2 + ["-fb_definition", "1-64/64filters", "-fea_ncepcoefs", "39"] + extra)
    assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and reason in str(ei.value), str(ei.value)


def test_ss_at_2048_points_with_wide_cepstra_is_refused_by_name():
    cfg = "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97 -vad burg -nr_mode fwss -fb_definition 1-40/40filters -fea_ncepcoefs 30".split()
    with pytest.raises(CtuError) as ei:
        ctucopy_amd.Engine(cfg)
    assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and "more than 24 cepstral values" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("bands,ncep,lifter", [(40, 39, 22), (64, 63, 22), (26, 30, 22), (40, 39, 0)])
def test_dct_table_is_the_references_formula_rounded_once(bands, ncep, lifter):
    """dctcFEA (src/fea/fea_impl.cc:92-127): wdct[i] = cos(3.1415926535898 i / 2B), c_i = sqrt(2/B) sum_k X_{k-1} wdct[(2k-1) i mod 4B],
    c_i *= 1 + L/2 sin(3.141592653589793 i / L) for i >= 1 when L > 1 - in float64, then one rounding to float."""
    cfg = C2 + ["-fb_definition", f"1-{bands}/{bands}filters", "-fea_ncepcoefs", str(ncep), "-fea_lifter", str(lifter)]
    got = config_table(cfg, "dct").reshape(ncep + 1, bands)
    wdct = np.cos(3.1415926535898 * np.arange(4 * bands, dtype=np.float64) / (2 * bands))
    i = np.arange(ncep + 1)[:, None]
    k = np.arange(1, bands + 1)[None, :]
    want = wdct[(2 * k - 1) * i % (4 * bands)] * np.sqrt(2.0 / bands)
    if lifter > 1:
        lift = 1 + (float(lifter) / 2) * np.sin(3.141592653589793 * (np.arange(ncep) + 1.0) / float(lifter))
        want[1:] *= lift[:, None]
    assert np.array_equal(got.astype(np.float32).view(np.uint32), want.astype(np.float32).view(np.uint32))
