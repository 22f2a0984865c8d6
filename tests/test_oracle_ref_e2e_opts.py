"""The oracle and the host-side helpers against the compiled reference over the rest of the option space: every case of tests/util.py's
REF_E2E_OPT_CASES and ref_e2e_file_cases() as tests/golden/ref_e2e_opts.npz holds it (tests/golden/make_ref_e2e_fixtures.py opts).

The rule is that of tests/test_oracle_ref_e2e.py, through its own checker: counts, header fields, VAD bytes and int16 samples equal, the
non-finite pattern identical, finite values within 2^-23 max(|ref|, 1).  The file cases hold the same rule on the floats inside the files
the reference wrote (HTK in both byte orders, ark, pfile, G.711 and wave input) and equality on every other byte of them.  CMVN: the
statistics text under the bound tests/test_cli.py uses for it, the applied rows under the one-ulp rule or, where the statistics' own
rounding is what is left, under the statistics' bound (see test_cmvn_helpers_match_the_reference_files)."""
import zlib

import numpy as np
import pytest

from oracle.oracle import Oracle, cmvn_apply, cmvn_slot_columns, cmvn_speakers, cmvn_stat_text, cmvn_stats
from tests.test_oracle_ref_e2e import ULP, check_oracle_case, reference_kind
from tests.util import (C1, REF_E2E_OPT_CASES, g711_codes, ref_e2e_file_cases, ref_e2e_inputs, ref_e2e_opts, ref_outputs, split_written_file,
                        synth_utt)

DAT_KIND = 6 | 0o20000 | 0o400 | 0o1000 | 0o100000     # MFCC_0_D_A_T as HTK defines it


@pytest.fixture(scope="module")
def fx():
    return ref_e2e_opts()


@pytest.fixture(scope="module")
def inputs():
    cache = {}
    return lambda name: cache.setdefault(name, ref_e2e_inputs(name))


@pytest.fixture(scope="module")
def file_cases():
    return ref_e2e_file_cases()


def test_the_fixture_holds_every_case_and_the_inputs_it_was_recorded_on(fx, inputs, file_cases):
    for name, (cfg, inp) in REF_E2E_OPT_CASES.items():
        assert int(fx[f"{name}__status"]) == 0, name       # none of these cases is one the reference dies on
        for i, u in enumerate(inputs(inp)):
            assert u.dtype == np.int16
            assert fx[f"{name}__{i}__input"].tolist() == [u.size, zlib.crc32(u.astype("<i2").tobytes())], (name, i)
    for name, (cfg, files, lst, outputs) in file_cases.items():
        assert int(fx[f"{name}__status"]) == 0, name
        assert fx[f"{name}__input"].tolist() == [zlib.crc32(files[f]) for f in sorted(files)], name
        assert {k.split("__file__")[1] for k in fx.files if k.startswith(name + "__file__")} == set(outputs), name
    assert {k.split("__")[0] for k in fx.files} == set(REF_E2E_OPT_CASES) | set(file_cases)


_FIGURES = {}


@pytest.mark.parametrize("name", list(REF_E2E_OPT_CASES))
def test_oracle_matches_the_compiled_reference(fx, inputs, name):
    _FIGURES[name] = check_oracle_case(fx, REF_E2E_OPT_CASES, inputs, name)
    print("ref e2e opts %s: %d finite values, %d not equal, worst %.3e" % ((name,) + _FIGURES[name]))


def test_agreement_figures_over_the_table(fx, inputs):
    # the figures DESIGN.md section 2 quotes: printed here, computed from the cases above (or again when this test runs alone)
    for name in REF_E2E_OPT_CASES:
        if name not in _FIGURES:
            _FIGURES[name] = check_oracle_case(fx, REF_E2E_OPT_CASES, inputs, name)
    total, unequal = sum(f[0] for f in _FIGURES.values()), sum(f[1] for f in _FIGURES.values())
    worst = max(f[2] for f in _FIGURES.values())
    print(f"ref e2e opts: {total - unequal} of {total} finite values equal, the other {unequal} within {worst:.3e}")
    assert worst <= ULP


def test_the_frameless_file_of_short3_is_one(fx):
    # short3 is there for the state a file without a frame hands on: no row at 16 kHz, two at 8 kHz
    for name, (cfg, inp) in REF_E2E_OPT_CASES.items():
        if inp == "short3" and f"{name}__1__rows" in fx.files:
            assert fx[f"{name}__1__rows"].shape[0] in ((0,) if cfg[cfg.index("-fs") + 1] == "16000" else (0, 2)), name


@pytest.mark.parametrize("name", ["post_dat", "post_dat_windows"])
def test_d_a_t_header_is_htk_s_t_bit_and_the_reference_s_is_its_decimal_misprint(fx, name):
    # the reference ORs decimal 100000 into the kind (src/io/out.cc:159), the project keeps HTK's T bit
    cfg, inp = REF_E2E_OPT_CASES[name]
    ours = Oracle(cfg).dims.htk_kind
    assert ours == DAT_KIND
    for i in range(2):
        recorded = int(fx[f"{name}__{i}__header"][3])
        assert recorded == (ours | 100000) & 0xFFFF == 0o123646
        assert recorded == reference_kind(ours, cfg)
    # no other case of the table is touched by the exception
    assert [n for n, (c, _) in REF_E2E_OPT_CASES.items() if reference_kind(1 << 15, c) != 1 << 15] == ["post_dat_windows", "post_dat"]


def _one_ulp(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), what
    err = np.abs(got[fin].astype(np.float64) - ref[fin]) / np.maximum(np.abs(ref[fin]), 1.0)
    print(f"ref e2e opts {what}: {int(fin.sum())} values, {int((got[fin] != ref[fin]).sum())} not equal, worst {float(err.max()) if err.size else 0.0:.3e}")
    assert err.size == 0 or err.max() <= ULP, (what, float(err.max()))


def _file_inputs(name, files):
    """int16 utterances the case's input files hold, in list order."""
    tab = ref_outputs()
    out = []
    for fn in sorted(files):
        if name == "file_alaw":
            out.append(tab["amulaw_a"][np.frombuffer(files[fn], np.uint8)])
        elif name == "file_mulaw":
            out.append(tab["amulaw_mu"][np.frombuffer(files[fn], np.uint8)])
        elif name == "file_wave":
            out.append(np.frombuffer(files[fn][44:], "<i2"))
        else:
            out.append(np.frombuffer(files[fn], "<i2"))
    return out


@pytest.mark.parametrize("name", ["file_ark", "file_pfile", "file_big_endian", "file_alaw", "file_mulaw", "file_wave"])
def test_oracle_matches_the_files_the_reference_wrote(fx, file_cases, name):
    cfg, files, lst, outputs = file_cases[name]
    big = name == "file_big_endian"
    ocfg = [a if not a.startswith(("ark=", "pfile=")) else "htk" for a in cfg]     # the rows are the writer's business, not the oracle's
    ocfg = [("raw" if a in ("alaw", "mulaw", "wave") else a) for a in ocfg]
    orc = Oracle(ocfg)
    want = [orc.process(u) for u in _file_inputs(name, files)]
    got = []
    for fn in outputs:
        rows, rest = split_written_file(fn, fx[f"{name}__file__{fn}"], big)
        got += rows
        if fn.startswith("out") and "." not in fn:        # an HTK header: the oracle's fields
            e = ">" if big else "<"
            n, period = np.frombuffer(rest, e + "u4", 2)
            size, kind = np.frombuffer(rest, e + "u2", 2, 8)
            assert (int(n), int(period), int(size), int(kind)) == (rows[0].shape[0], orc.dims.period, 4 * orc.dims.D, orc.dims.htk_kind), (name, fn)
    assert len(got) == len(want), name
    for i, (g, w) in enumerate(zip(got, want)):
        _one_ulp(w, g, f"{name}[{i}]")
    if name == "file_ark":
        ark, scp = bytes(fx["file_ark__file__out.ark"]), bytes(fx["file_ark__file__out.scp"]).decode().split("\n")
        offs = [int(l.split(":")[1]) for l in scp if l]
        assert [l.split(":")[0] for l in scp if l] == ["utt0 out.ark", "utt1 out.ark"]
        assert all(ark[o - 5:o] == b"utt%d" % i + b" " for i, o in enumerate(offs)) and all(ark[o:o + 5] == b"\0BFM " for o in offs)


CMVN_SPK = ["spkA", "spkB", "spkB"]


@pytest.mark.parametrize("name", ["file_cmvn", "file_cmvn_da"])
def test_cmvn_helpers_match_the_reference_files(fx, file_cases, name):
    cfg, files, lst, outputs = file_cases[name]
    base = [a for a in cfg[:-2]]                                     # the chain without -apply_cmvn <file>
    orc = Oracle(base)
    rows = [orc.process(u) for u in _file_inputs(name, files)]
    ids, spk = cmvn_speakers(CMVN_SPK)
    cols = cmvn_slot_columns(12, 3 if "-fea_delta" in cfg else 1)
    mean, var, _ = cmvn_stats(rows, spk, len(ids), cols)
    text, want = bytes(fx[f"{name}__file__stat"]).decode(), cmvn_stat_text(ids, mean, var)
    label = lambda t: [l.split("\t")[0] for l in t.splitlines()]
    assert label(text) == label(want)
    vals = lambda t: np.array([[float(v) for v in l.split("\t")[1].split()] for l in t.splitlines() if "\t" in l])
    got_vals, want_vals = vals(text), vals(want)
    stat_bound = 2e-6 + 1e-6 * np.abs(want_vals).max()
    print(f"ref e2e opts {name}: statistics differ by {np.abs(got_vals - want_vals).max():.3e} at the most (bound {stat_bound:.3e})")
    assert got_vals.shape == want_vals.shape == (2 * len(ids), len(cols)) and np.abs(got_vals - want_vals).max() <= stat_bound
    # The applied rows: the reference divides by the variance it holds in double, the helpers by theirs - summed over float32 rows instead
    # of the doubles behind them - so (F - mean) / var carries the statistics' relative rounding, a few 1e-7 of |row| <= 10 (DESIGN.md
    # section 2): the rows are held to the statistics' bound, 2e-6 + 1e-6 max|ref row|, and the one-ulp figures are printed beside it.
    worst_abs = worst_ulp = row_bound = 0.0
    for i in range(3):
        got, rest = split_written_file(f"out{i}", fx[f"{name}__file__out{i}"])
        n, period = np.frombuffer(rest, "<u4", 2)
        size, kind = np.frombuffer(rest, "<u2", 2, 8)
        assert (int(n), int(period), int(size), int(kind)) == (rows[i].shape[0], orc.dims.period, 4 * orc.dims.D, orc.dims.htk_kind), (name, i)
        mine = cmvn_apply(rows[i], spk[i], mean, var, cols)
        assert mine.shape == got[0].shape and np.isfinite(got[0]).all()
        d = np.abs(mine.astype(np.float64) - got[0])
        row_bound = max(row_bound, 2e-6 + 1e-6 * float(np.abs(got[0]).max()))
        worst_abs, worst_ulp = max(worst_abs, float(d.max())), max(worst_ulp, float((d / np.maximum(np.abs(got[0]), 1.0)).max()))
    print(f"ref e2e opts {name}: applied rows differ by {worst_abs:.3e} absolute, {worst_ulp:.3e} against max(|ref|, 1) (one ulp: {ULP:.3e}; bound {row_bound:.3e})")
    assert worst_abs <= row_bound
