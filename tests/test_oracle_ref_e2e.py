"""The oracle against the compiled reference, end to end: every case of tests/util.py's REF_E2E_CASES as tests/golden/ref_e2e.npz holds it
(recorded by tests/golden/make_ref_e2e_fixtures.py from the reference's own sources, built against oracle/fftw_standin.cc).

Row counts, HTK header fields, VAD bytes and int16 samples are equal; the non-finite pattern is identical; finite values lie within
2^-23 max(|ref|, 1) element-wise: both sides are double chains rounded once to float32, so a different rounding inside the FFT moves a value
by one float32 ulp at the most.  Cases the reference died on assert nothing about values, only that DESIGN.md section 7 lists them."""
import os
import re
import zlib

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.util import EDGE_INPUTS, REF_E2E_CASES, REF_E2E_OPT_CASES, ref_e2e, ref_e2e_inputs, ref_e2e_opts, zeros_mid_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def fx():
    return ref_e2e()


@pytest.fixture(scope="module")
def inputs():
    cache = {}
    return lambda name: cache.setdefault(name, ref_e2e_inputs(name))


def _is_signal(cfg):
    return cfg[cfg.index("-format_out") + 1] == "raw"


def _has_vad_file(cfg):
    return any(a.startswith("-vad_") for a in cfg)


def test_the_fixture_holds_every_case_and_the_inputs_it_was_recorded_on(fx, inputs):
    for name, (cfg, inp) in REF_E2E_CASES.items():
        assert f"{name}__status" in fx.files, name
        if int(fx[f"{name}__status"]):
            assert not [k for k in fx.files if k.startswith(name + "__") and not k.endswith("__status")], name
            continue
        for i, u in enumerate(inputs(inp)):
            assert u.dtype == np.int16
            assert fx[f"{name}__{i}__input"].tolist() == [u.size, zlib.crc32(u.astype("<i2").tobytes())], (name, i)
    assert {k.split("__")[0] for k in fx.files} == set(REF_E2E_CASES)


def test_the_reference_crashes_are_the_ones_the_design_lists(fx):
    # both tables: every status key of ref_e2e.npz and ref_e2e_opts.npz (the file cases of the second among them)
    both = [(k[:-len("__status")], int(f[k])) for f in (fx, ref_e2e_opts()) for k in f.files if k.endswith("__status")]
    assert {n for n, _ in both} >= set(REF_E2E_CASES) | set(REF_E2E_OPT_CASES) and len(both) == len({n for n, _ in both})
    crashed = {name: status for name, status in both if status}
    assert crashed and set(crashed.values()) <= {139, 134, 124}
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("\n## 7"):]
    section = section[:section.index("\n## ", 1)] if "\n## " in section[1:] else section
    listed = {m.group(1): int(m.group(2)) for m in re.finditer(r"`ref_e2e:(\w+)` \(exit status (\d+)\)", section)}
    assert listed == crashed


# The one header field in which the project deviates from the reference on purpose: with -fea_delta d_a_t the reference
# ORs the T qualifier in as DECIMAL 100000 (src/io/out.cc:159; the lines above it are octal), which sets HTK's C and N bits too and turns
# the base kind into 38; the project writes HTK's T bit, 0o100000.  tests/test_oracle_ref_e2e_opts.py pins it from both sides.
def reference_kind(ours, cfg):
    if "-fea_delta" in cfg and cfg[cfg.index("-fea_delta") + 1] == "d_a_t":
        assert ours & 0o100000
        return (ours | 100000) & 0xFFFF
    return ours


@pytest.mark.parametrize("name", list(REF_E2E_CASES))
def test_oracle_matches_the_compiled_reference(fx, inputs, name):
    check_oracle_case(fx, REF_E2E_CASES, inputs, name)


def check_oracle_case(fx, cases, inputs, name):
    """The rule of this module on one case: returns (finite values, values not equal, worst error) for the figures DESIGN.md quotes."""
    cfg, inp = cases[name]
    if int(fx[f"{name}__status"]):
        return 0, 0, 0.0   # the reference died: test_the_reference_crashes_are_the_ones_the_design_lists holds the list
    utts = inputs(inp)
    count = unequal = 0
    worst = 0.0
    orc = Oracle(cfg)
    if _is_signal(cfg):
        for i, u in enumerate(utts):     # one Oracle over the list: the *ss modes go on from the vector the previous file left
            got, ref = orc.enhance(u), fx[f"{name}__{i}__pcm"]
            assert got.shape == ref.shape and np.array_equal(got, ref), (name, i)
        return 0, 0, 0.0
    want_vad = _has_vad_file(cfg)
    out = orc.process_list(utts, want_vad=want_vad)
    for i, o in enumerate(out):
        rows, vad = o if want_vad else (o, None)
        ref, hdr = fx[f"{name}__{i}__rows"], fx[f"{name}__{i}__header"]
        d = orc.dims
        assert rows.shape == ref.shape, (name, i)
        # -fea_trap: the writer renames o->fea_kind to "spec" at its first frame (src/io/out.cc:182), so the headers of a list's later files
        # carry base kind 8 - the command-line host writes the same (ctucopy_amd/host/main.cc)
        kind = (d.htk_kind & ~0o77) | 8 if "-fea_trap" in cfg and i > 0 else d.htk_kind
        assert hdr.tolist() == [ref.shape[0], d.period, 4 * d.D, reference_kind(kind, cfg)], (name, i)
        if want_vad:
            assert np.array_equal(vad, fx[f"{name}__{i}__vad"]), (name, i)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(rows), fin), (name, i)
        assert np.array_equal(np.isnan(rows), np.isnan(ref)) and np.array_equal(rows[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), (name, i)
        err = np.abs(rows[fin].astype(np.float64) - ref[fin]) / np.maximum(np.abs(ref[fin]), 1.0)
        assert err.size == 0 or err.max() <= ULP, (name, i, float(err.max()))
        count, unequal = count + int(fin.sum()), unequal + int((rows[fin] != ref[fin]).sum())
        worst = max(worst, float(err.max()) if err.size else 0.0)
    return count, unequal, worst


def _zero_block_frames(cfg, n, rows):
    """Frames of zeros_mid(n) wholly inside the zero block (with pre-emphasis: the sample in front of the frame too)."""
    opt = {k: v for k, v in zip(cfg[:-1], cfg[1:]) if k.startswith("-")}
    fs = int(opt["-fs"])
    window, shift = int(float(opt.get("-w", 25)) * fs / 1000), int(float(opt.get("-s", 10)) * fs / 1000)
    a, z, _ = zeros_mid_parts(n)
    starts = np.arange(rows) * shift
    return (starts - (1 if float(opt.get("-preem", 0)) > 0 else 0) >= a) & (starts + window <= a + z)


@pytest.mark.parametrize("name", [n for n, (c, i) in REF_E2E_CASES.items() if i.startswith("edge") and not _is_signal(c)])
def test_conditions_on_the_edge_rows_of_the_reference(fx, name):
    # what the GPU tests rely on: finite targets on the seven finite-valued inputs; on zeros_mid non-finite rows exactly where a frame holds
    # nothing but zeros (the logarithm of an empty band), at most a quarter of the file
    cfg, inp = REF_E2E_CASES[name]
    n = int(inp[len("edge"):])
    for i, g in enumerate(EDGE_INPUTS):
        rows = fx[f"{name}__{i}__rows"]
        bad = ~np.isfinite(rows).all(axis=1)
        if g != "zeros_mid":
            assert not bad.any(), (name, g)
        else:
            assert np.array_equal(bad, _zero_block_frames(cfg, n, rows.shape[0])), name
            assert 0 < bad.sum() <= rows.shape[0] / 4, (name, int(bad.sum()), rows.shape[0])


def test_the_edge_signal_output_does_saturate(fx):
    # edge_i is there for the int16 saturation of the overlap-add: the reference does write samples at a rail (it clamps to +-32767)
    rail = sum(int((np.abs(fx[f"edge_i__{i}__pcm"].astype(np.int32)) >= 32767).sum()) for i in range(len(EDGE_INPUTS)))
    assert rail > 0
