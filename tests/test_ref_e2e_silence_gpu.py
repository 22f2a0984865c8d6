"""The engine against the compiled reference on digital silence through the stateful chains: tests/util.py's REF_E2E_SILENCE_CASES as
tests/golden/ref_e2e_silence.npz holds them (recorded by tests/golden/make_ref_e2e_fixtures.py silence).  Every case is one list of two
files: speech around a block of zeros (a muted telephone channel), then plain speech, which shows what the first file hands on.

The rules are those of tests/test_ref_e2e_gpu.py, through its own functions and unchanged: on the rows the reference left finite, 1e-4
element-wise for the well-conditioned class, 1e-3 element-wise and 1e-4 of the row's largest value otherwise (2fwss under the rule of
tests/test_ref_e2e_opts_gpu.py, as it stands); a row the reference left non-finite has a non-finite value on the device; every VAD byte
equal, the list as one process's; samples within 2 LSB, mean below 0.3.  New here: A ROW THE REFERENCE LEFT FINITE IS FINITE ON THE
DEVICE.  The reference's sequential double code and fp32 GPU code differ on non-finite operands - a padded tap of weight 0 on a
neighbouring frame is 0 x -inf = NaN, the low half of an fp16 split of -inf is NaN, v_max_f32 / v_min_f32 / v_med3 drop a NaN where
`a > b ? a : b` keeps one side, a scan or an underflowing p^k "recovers" where m <- p m + (1 - p) x does not - and the rows around the
block and the whole second file are where that shows.  `sil_c4` is what the reference dies on: the engine runs
on and is held to the oracle, rows and every VAD byte of both files.  Every test prints its figures before it asserts.
"""
import numpy as np
import pytest

from tests.test_ref_e2e_gpu import Engine, VAD_FILTER_ORDER, _assert_rows, _assert_samples  # noqa: F401  (Engine: the module's fixture)
from tests.test_ref_e2e_opts_gpu import _assert_2fwss_rows
from tests.util import REF_E2E_SILENCE_CASES, REF_E2E_SILENCE_NONFINITE, SILENCE_DIES, ref_e2e_inputs, ref_e2e_silence

pytestmark = pytest.mark.gpu

FX = ref_e2e_silence()
ROW_CASES = [n for n in REF_E2E_SILENCE_CASES if n in REF_E2E_SILENCE_NONFINITE]
# the kernel family each case is there for, as far as ctu_engine_kernel_name shows it (the front end; the row stages behind it - trapdct's
# MFMA kernels, the delta / stacking / CMS chains, vad_decide_kernel - follow from the command line)
KERNEL = {
    "sil_c4": "frontend_kernel<13, DCTC, MODE 1, exten, MD, VF>",           # exten + the fused Burg-cepstral detector, two frames a transform
    "sil_c4_novad": "frontend_kernel<13, DCTC, MODE 1, exten, MD>",
    "sil_fwss": "frontend_kernel<13, DCTC, MODE 0, plain, MD, SS>",
    "sil_2fwss_8k": "frontend_kernel<13, DCTC, MODE 1, plain, MD, SS>",
    "sil_hwss_8k": "frontend_kernel<13, DCTC, MODE 1, plain, MD, SS>",
    "sil_trapdct51": "frontend_kernel<13, BANDS, MODE 0, plain>",           # log-mel bands into the trapdct kernels
    "sil_da_zexp_e": "frontend_kernel<13, DCTC, MODE 0, full>",
    "sil_trap9": "frontend_kernel<13, DCTC, MODE 0, plain, MD>",
    "sil_zblock30": "frontend_kernel<13, DCTC, MODE 0, plain, MD>",
    "sil_vad_energy_dyn": "frontend_kernel<13, DCTC, MODE 0, full>",
    "sil_vad_energy_perc": "frontend_kernel<13, DCTC, MODE 0, full>",
    "sil_vad_fea_adapt": "frontend_kernel<13, DCTC, MODE 0, plain>",        # the criterion reads finished rows: vad_decide_kernel
    "sil_lpc12": "frontend_kernel<13, LPD, MODE 0, full>",                  # the double LP tail
    "sil_plp": "frontend_kernel<13, LP, MODE 0, inld, MD>",
    "sil_logspec_e": "frontend_kernel<13, BANDS, MODE 0, full>",
    "sil_spec": "frontend_kernel<13, BANDS, MODE 0, plain>",
    "sil_sig_fwss": "frontend_kernel<13, BANDS, MODE 0, full, SS, SY>",
    "sil_m48_w64": "bigfft_kernel<16>",
}

_INPUTS = {}


def inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = ref_e2e_inputs(name)
        for u in _INPUTS[name]:
            u.setflags(write=False)
    return _INPUTS[name]


def _check_file(name, i, cfg, g, ref, failed, what="reference"):
    """The rules of this module on one file's rows; failures are collected so that every file's figures are printed first."""
    assert g.shape == ref.shape and g.dtype == np.float32, (name, i, g.shape, ref.shape)
    fin, dev = np.isfinite(ref).all(axis=1), np.isfinite(g).all(axis=1)
    lost, kept = np.flatnonzero(fin & ~dev), np.flatnonzero(~fin & dev)
    print(f"ref e2e silence {name}[{i}]: {ref.shape[0]} rows, non-finite in the {what} {np.flatnonzero(~fin).tolist()}, on the device {np.flatnonzero(~dev).tolist()}; "
          f"finite in the {what} but not on the device {lost.tolist()}, non-finite in the {what} but finite on the device {kept.tolist()}")
    try:
        if "2fwss" in cfg:
            _assert_2fwss_rows(g[fin], ref[fin], f"{name}[{i}]")
        else:
            _assert_rows(g[fin], ref[fin], cfg, f"{name}[{i}]")
    except AssertionError as e:
        failed.append(str(e))
    if lost.size:
        failed.append(f"{name}[{i}]: rows {lost.tolist()} are finite in the {what} and not on the device")
    if kept.size:
        failed.append(f"{name}[{i}]: rows {kept.tolist()} are non-finite in the {what} and finite on the device")


@pytest.mark.parametrize("name", ROW_CASES)
def test_silence_case_matches_the_compiled_reference(Engine, name):
    cfg, inp = REF_E2E_SILENCE_CASES[name]
    utts = inputs(inp)
    eng = Engine(cfg)     # one engine over the list: what the first file hands on is what the second file is there for
    assert eng.kernel_name() == KERNEL[name], eng.kernel_name()
    has_vad = f"{name}__0__vad" in FX.files
    if has_vad:
        got, vads = eng.extract(utts, want_vad=True, as_list_of_one_process=VAD_FILTER_ORDER)
    else:
        got, vads = eng.extract(utts), None
    hdr = FX[f"{name}__0__header"]
    assert [int(hdr[1]), int(hdr[2]), int(hdr[3])] == [eng.dims.htk_period, 4 * eng.dims.row_floats, eng.dims.htk_kind], (name, hdr)
    failed = []
    for i, g in enumerate(got):
        ref = FX[f"{name}__{i}__rows"]
        if has_vad:
            v, rv = np.asarray(vads[i]), FX[f"{name}__{i}__vad"]
            differ = np.flatnonzero(v != rv).tolist() if v.size == rv.size else None
            print(f"ref e2e silence {name}[{i}]: {v.size} VAD bytes, differ at {differ}, {int((rv == ord('1')).sum())} ones")
            if not np.array_equal(v, rv):
                failed.append(f"{name}[{i}]: VAD bytes differ at {differ}")
        _check_file(name, i, cfg, g, ref, failed)
    want = REF_E2E_SILENCE_NONFINITE[name]
    bad = ~np.isfinite(FX[f"{name}__0__rows"]).all(axis=1)
    assert bad.any() == (want[0] is not None)          # (the block shows in the target, or the case is one whose silent frames are finite)
    assert not failed, failed


def test_c4_runs_on_where_the_reference_aborts_and_is_the_oracle_s(Engine):
    from oracle.oracle import Oracle
    name = "sil_c4"
    cfg, inp = REF_E2E_SILENCE_CASES[name]
    assert int(FX[f"{name}__status"]) == SILENCE_DIES[name] == 134
    utts = inputs(inp)
    eng = Engine(cfg)
    assert eng.kernel_name() == KERNEL[name], eng.kernel_name()
    got, vads = eng.extract(utts, want_vad=True, as_list_of_one_process=VAD_FILTER_ORDER)
    want = Oracle(cfg).process_list(utts, want_vad=True)
    failed, ones, total = [], 0, 0
    for i, ((ref, rv), g, v) in enumerate(zip(want, got, vads)):
        v = np.asarray(v)
        differ = np.flatnonzero(v != rv).tolist() if v.size == rv.size else None
        print(f"ref e2e silence {name}[{i}]: {v.size} VAD bytes, differ from the oracle's at {differ}, {int((rv == ord('1')).sum())} ones")
        if not np.array_equal(v, rv):
            failed.append(f"{name}[{i}]: VAD bytes differ at {differ}")
        _check_file(name, i, cfg, g, ref, failed, what="oracle")
        ones, total = ones + int((rv == ord("1")).sum()), total + rv.size
    assert 0 < ones < total
    assert not np.isfinite(want[0][0]).all() and np.isfinite(want[1][0]).all()
    assert not failed, failed


def test_fp32_trapdct_kernel_on_silence_is_the_oracle_s(Engine):
    """sil_trapdct51 has 23 bands and runs trapdct_split16_kernel.  With the preset's 26 bands the offline run launches the exact-fp32
    trapdct_mfma_kernel, whose 31 taps are padded to 26 tap groups of weight zero that fetch real frames up to 88 ahead.  No recording
    holds this chain on silence: the target is the oracle, which is the reference's on sil_trapdct51 to the last bit
    (tests/test_oracle_ref_e2e_silence.py).  Rows 14 .. 59 of 73 hold an all-zero frame in their context of 31."""
    from oracle.oracle import Oracle
    from tests.util import C2
    cfg = C2 + ["-fea_kind", "trapdct,31,8"]
    utts = inputs("sil12000")
    eng = Engine(cfg)
    assert eng.kernel_name() == "frontend_kernel<13, BANDS, MODE 0, plain>" and eng.dims.row_floats == 26 * 8
    got = eng.extract(utts)
    orc = Oracle(cfg)
    failed = []
    for i, (g, u) in enumerate(zip(got, utts)):
        ref = orc.process(u)
        if i == 0:
            assert np.flatnonzero(~np.isfinite(ref).all(axis=1)).tolist() == list(range(14, 60)) and ref.shape[0] == 73
        else:
            assert np.isfinite(ref).all()
        _check_file("trapdct31_26bands", i, cfg, g, ref, failed, what="oracle")
    assert not failed, failed


def test_signal_output_behind_fwss_matches_the_compiled_reference(Engine):
    name = "sil_sig_fwss"
    cfg, inp = REF_E2E_SILENCE_CASES[name]
    eng = Engine(cfg)
    assert eng.dims.signal_out == 1 and eng.kernel_name() == KERNEL[name], eng.kernel_name()
    failed = []
    for i, g in enumerate(eng.enhance(inputs(inp))):
        try:
            _assert_samples(g, FX[f"{name}__{i}__pcm"], f"{name}[{i}]")
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, failed
