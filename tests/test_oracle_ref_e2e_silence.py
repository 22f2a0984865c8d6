"""The oracle against the compiled reference on digital silence through the stateful chains: every case of tests/util.py's
REF_E2E_SILENCE_CASES as tests/golden/ref_e2e_silence.npz holds it (tests/golden/make_ref_e2e_fixtures.py silence).  A muted telephone
channel is a run of one code; in mu-law 0xFF and 0x7F both expand to 0, and on an all-zero frame the reference takes the logarithm of
an empty band.  Every stage that carries state from frame to frame then decides how far the -inf / NaN spreads: the smoothing chains,
the exponential and block CMS, the VAD's thresholds, the noise estimates of hwss / fwss / 2fwss, Levinson's recursion.

The rule is that of tests/test_oracle_ref_e2e.py, through its own checker: counts, header fields, VAD bytes and int16 samples equal, the
non-finite pattern identical, finite values within 2^-23 max(|ref|, 1); VAD lists go through the oracle's list mode.  The conditions the
GPU tests rely on (tests/util.py's check_silence_conditions) are asserted on the recording.  `sil_c4` is what the reference dies on
(Burg.h:72, den != 0.0, on the first silent frame: DESIGN.md section 7): its status is asserted, and the oracle's walk - the target of
the GPU test - is held to finite rows outside the silent frames and to decisions of both kinds."""
import os
import re
import zlib

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.test_oracle_ref_e2e import ULP, check_oracle_case
from tests.util import (REF_E2E_OPT_CASES, REF_E2E_SILENCE_CASES, REF_E2E_SILENCE_NONFINITE, SILENCE_DIES, SILENCE_VAD_ONES, GOLDEN,
                        check_silence_conditions, ref_e2e_inputs, ref_e2e_silence, zero_block_frames)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAN = [n for n in REF_E2E_SILENCE_CASES if n not in SILENCE_DIES]


@pytest.fixture(scope="module")
def fx():
    return ref_e2e_silence()


@pytest.fixture(scope="module")
def inputs():
    cache = {}
    return lambda name: cache.setdefault(name, ref_e2e_inputs(name))


def test_the_fixture_holds_every_case_and_the_inputs_it_was_recorded_on(fx, inputs):
    for name, (cfg, inp) in REF_E2E_SILENCE_CASES.items():
        assert int(fx[f"{name}__status"]) == SILENCE_DIES.get(name, 0), name
        if name in SILENCE_DIES:
            assert not [k for k in fx.files if k.startswith(name + "__") and not k.endswith("__status")], name
            continue
        utts = inputs(inp)
        assert len(utts) == 2 and utts[1].size == utts[0].size // 2
        for i, u in enumerate(utts):
            assert u.dtype == np.int16
            assert fx[f"{name}__{i}__input"].tolist() == [u.size, zlib.crc32(u.astype("<i2").tobytes())], (name, i)
    assert {k.split("__")[0] for k in fx.files} == set(REF_E2E_SILENCE_CASES)
    assert os.path.getsize(os.path.join(GOLDEN, "ref_e2e_silence.npz")) <= os.path.getsize(os.path.join(GOLDEN, "ref_e2e_opts.npz"))


def test_what_the_reference_dies_on_is_in_the_design(fx):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("\n## 7"):]
    section = section[:section.index("\n## ", 1)] if "\n## " in section[1:] else section
    listed = {m.group(1): int(m.group(2)) for m in re.finditer(r"`ref_e2e_silence:(\w+)` \(exit status (\d+)\)", section)}
    assert listed == SILENCE_DIES == {n: int(fx[f"{n}__status"]) for n in REF_E2E_SILENCE_CASES if int(fx[f"{n}__status"])}


_FIGURES = {}


@pytest.mark.parametrize("name", RAN)
def test_oracle_matches_the_compiled_reference(fx, inputs, name):
    _FIGURES[name] = check_oracle_case(fx, REF_E2E_SILENCE_CASES, inputs, name)
    print("ref e2e silence %s: %d finite values, %d not equal, worst %.3e" % ((name,) + _FIGURES[name]))
    assert _FIGURES[name][2] <= ULP


@pytest.mark.parametrize("name", [n for n in RAN if n in REF_E2E_SILENCE_NONFINITE])
def test_conditions_on_the_rows_of_the_reference(fx, name):
    cfg, inp = REF_E2E_SILENCE_CASES[name]
    ahead, behind = check_silence_conditions(name, cfg, fx[f"{name}__0__rows"], fx[f"{name}__1__rows"])
    print(f"ref e2e silence {name}: {ahead} finite rows ahead of the block, {behind} behind, {fx[f'{name}__1__rows'].shape[0]} rows in the second file")


def test_every_case_with_rows_has_its_conditions():
    assert set(REF_E2E_SILENCE_NONFINITE) == set(RAN) - {"sil_sig_fwss"}


@pytest.mark.parametrize("name", list(SILENCE_VAD_ONES))
def test_the_vad_cases_decide_both_ways(fx, name):
    # a test on an all-zero byte string would be weak (-vad_thr_mode adapt on the energy criterion gives no ones at all on this input)
    v = fx[f"{name}__0__vad"]
    assert v.size == 73 and int((v == ord("1")).sum()) == SILENCE_VAD_ONES[name] and set(np.unique(v)) == {ord("0"), ord("1")}
    v1 = fx[f"{name}__1__vad"]
    assert v1.size == fx[f"{name}__1__rows"].shape[0] and set(np.unique(v1)) <= {ord("0"), ord("1")}


def test_the_signal_case_holds_the_samples_of_both_files(fx, inputs):
    utts = inputs(REF_E2E_SILENCE_CASES["sil_sig_fwss"][1])
    for i, u in enumerate(utts):
        pcm = fx[f"sil_sig_fwss__{i}__pcm"]
        assert pcm.dtype == np.int16 and 0 < pcm.size <= u.size and np.abs(pcm.astype(np.int32)).max() > 1000


def test_the_walk_of_the_oracle_where_the_reference_aborts(fx, inputs):
    # C4 on zeros_mid: Burg's recursion divides by a zero denominator on the first silent frame, and the reference asserts.  The oracle
    # runs on (the engine does too, and is held to the oracle: tests/test_ref_e2e_silence_gpu.py), so what it gives is pinned here
    cfg, inp = REF_E2E_SILENCE_CASES["sil_c4"]
    assert int(fx["sil_c4__status"]) == 134
    utts = inputs(inp)
    out = Oracle(cfg).process_list(utts, want_vad=True)
    rows, vad = out[0]
    silent = zero_block_frames(cfg, utts[0].size, rows.shape[0])
    bad = ~np.isfinite(rows).all(axis=1)
    print(f"ref e2e silence sil_c4: oracle rows {rows.shape}, non-finite {np.flatnonzero(bad).tolist()}, silent frames {np.flatnonzero(silent).tolist()}, "
          f"{int((vad == ord('1')).sum())} ones of {vad.size}")
    assert rows.shape[0] == vad.size == REF_E2E_SILENCE_NONFINITE["sil_c4_novad"][2] and silent.sum() >= 2
    assert not bad[~silent].any()
    assert set(np.unique(vad)) == {ord("0"), ord("1")}
    rows1, vad1 = out[1]
    assert rows1.shape[0] == vad1.size > 10 and np.isfinite(rows1).all()


def test_the_table_adds_to_the_option_space_not_over_it():
    assert not set(REF_E2E_SILENCE_CASES) & set(REF_E2E_OPT_CASES)
