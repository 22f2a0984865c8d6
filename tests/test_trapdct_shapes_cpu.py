"""Offline TRAP-DCT over its shape space, the part that needs no GPU (the cases: tests/trap_cases.py; the GPU part:
tests/test_trapdct_shapes.py).

  - the launch shape is stated once on the host (trap_path, layout_constants.h; ctu_config_table(..., "trap_path")): which kernel runs at
    the boundaries the cases sit on, and that every accepted configuration asks for dynamic LDS its launch is entitled to;
  - config_table(cfg, "trap") is the reference's operator: contracted in float64 with the oracle's log-mel values it gives the oracle's
    trapdct rows to their float32 rounding;
  - the inputs of the GPU cases leave the kernel half of the parity bound: the float32 rounding of the log-mel rows alone costs at most
    0.5e-4;
  - the comparator of the GPU test sees a wrong kernel: a restatement of the contraction with one of six faults fails it."""
import numpy as np
import pytest

from ctucopy_amd import CtuError, config_table
from oracle.oracle import Oracle
from tests.trap_cases import (CASES, FAULTS, LARGEST, M1_26, M1_64, M2_26, M2_64, SHIFT, SMALLEST, SPLIT16, TOL, WINDOW, case_id, contract, frame_counts,
                              logspec_cfg, n_bands, operation_error, trap_cfg, utterances)
from tests.util import C2, C5

LDS_DEFAULT, LDS_RAISED = 64 * 1024, 160 * 1024   # what a launch gets as it is, and with the kernel's limit raised first


def _path(bank, traplen, ndct):
    p = config_table(C2 + ["-fb_definition", bank, "-fea_kind", "trapdct,%d,%d" % (traplen, ndct)], "trap_path")
    assert p.shape == (6,)
    return tuple(int(v) for v in p)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_case_runs_on_the_kernel_it_names(case):
    p = _path(*case[1:])
    assert p[:3] == case[0] and p[5] == 1
    assert p[4] == (p[3] > LDS_DEFAULT) and p[3] <= LDS_RAISED
    assert frame_counts(case[2])[0] == (case[2] + 1) // 2
    assert (config_table(trap_cfg(case), "frontend") == config_table(logspec_cfg(case), "frontend")).all()   # one front end writes both


def test_the_boundaries_of_the_kernels():
    assert _path("23filters", 101, 16)[:3] == SPLIT16 == _path(*CASES[0][1:])[:3] and C5[-1] == "trapdct,101,16"
    # the split kernel ends at 113 frames, 24 bands, 16 coefficients
    assert _path("24filters", 113, 16)[:3] == SPLIT16
    assert _path("24filters", 115, 16)[:3] == M1_64 and _path("25filters", 113, 16)[:3] == M1_64 and _path("24filters", 113, 17)[:3] == M2_64
    assert _path("23filters", 101, 17)[:3] == M2_26 and _path("25filters", 31, 16)[:3] == M1_26
    # the short fp32 instantiation ends at 26 tap groups; two row blocks from 17 coefficients on
    assert _path("26filters", 103, 16)[:3] == M1_26 and _path("26filters", 105, 16)[:3] == M1_64
    assert _path("26filters", 103, 17)[:3] == M2_26 and _path("26filters", 105, 17)[:3] == M2_64
    assert _path("26filters", 51, 32)[:3] == M2_26 and _path("50filters", 255, 32)[:3] == M2_64
    # the bytes: the split kernel's tile, centre values, fragment buffers and mask; the fp32 kernel's tile of 64 + 4 nsm frames and mask
    assert _path("24filters", 113, 16)[3] == 2 * 24 * 264 * 2 + 24 * 4 + 2 * 512 * 16 + (24 * 8 + 4) * 4
    assert _path("26filters", 31, 5)[3] == (64 + 4 * 26) * 27 * 4 + (26 * 10 + 1) * 4
    assert _path("26filters", 105, 16)[3] == (64 + 4 * 27) * 27 * 4 + (26 * 10 + 1) * 4
    # 50 and 51 bands pass 64 KiB from 245 frames (62 tap groups) on, the mask behind the tile: the launch raises the kernel's limit first
    assert _path("1-51/51filters", 245, 17)[3:] == (65692, 1, 1) and _path("50filters", 255, 32)[3:] == (67284, 1, 1)
    assert _path("1-51/51filters", 255, 32)[3:] == (67324, 1, 1)
    assert _path("1-51/51filters", 243, 17)[3:] == ((64 + 4 * 61) * 51 * 4 + 511 * 4, 0, 1) and _path("1-49/49filters", 255, 32)[4:] == (0, 1)
    # what is refused stays refused
    assert _path("1-52/52filters", 31, 16)[5] == 0 and _path("1-51/51filters", 31, 16)[5] == 1
    with pytest.raises(CtuError):
        config_table(C2, "trap_path")


def test_every_accepted_shape_asks_for_lds_its_launch_is_entitled_to():
    """Every odd traplen 3 .. 255 x 1 .. 51 bands x ndct in {1, 16, 17, 32} (ndct < traplen, the reference's rule), and 52 bands refused."""
    big = []
    for B in range(1, 53):
        bank = "1-%d/%dfilters" % (B, B)
        for traplen in range(3, 256, 2):
            for ndct in (1, 16, 17, 32):
                if ndct >= traplen:
                    continue
                split16, nrb, nsm, lds, raised, accepted = _path(bank, traplen, ndct)
                assert accepted == (B <= 51), (B, traplen, ndct)
                if not accepted:
                    continue
                assert 0 < lds <= LDS_RAISED and (lds <= LDS_DEFAULT or raised), (B, traplen, ndct, lds, raised)
                assert split16 == (ndct <= 16 and traplen <= 113 and B <= 24) and (split16 or (nrb, nsm) == (1 if ndct <= 16 else 2, 26 if traplen <= 104 else 64))
                if raised:
                    big.append((B, traplen))
    assert sorted(set(big)) == [(B, t) for B in (50, 51) for t in range(245, 256, 2)]


def _oracle_logmel64(cfg, x, T):
    """The oracle's log-mel values of x as it holds them, in float64: frame t is the last frame of the prefix that ends with it."""
    orc = Oracle(cfg)
    rows = []
    for t in range(T):
        orc.process(x[:WINDOW + t * SHIFT])
        rows.append(np.log(orc.last_fbank()))
    return np.array(rows)


@pytest.mark.parametrize("case", [CASES[3], CASES[4], CASES[9], CASES[13], CASES[18]], ids=case_id)
def test_the_trap_table_is_the_references_operator(case):
    """fea_trap.cc:84-108: mean removal, Hamming 0.54 - 0.46 cos(2 pi j / (traplen - 1)), REDFT10, coefficient 0 dropped - folded into
    config_table(cfg, "trap").  Contracted in float64 with the oracle's own float64 log-mel values it gives the oracle's trapdct rows to the
    rounding of those rows to float32 (half an ulp: 2^-24 relative; 1e-10 for the order of the float64 sums, partial sums of a few hundred
    over 255 taps at 1.1e-16 each)."""
    _, bank, traplen, ndct = case
    T = (traplen + 1) // 2 + 9
    x = utterances(case)[-1][:WINDOW + (T - 1) * SHIFT + 7]
    ref = Oracle(trap_cfg(case)).process(x)
    L64 = _oracle_logmel64(logspec_cfg(case), x, T)
    assert ref.shape == (T, n_bands(bank) * ndct) and L64.shape == (T, n_bands(bank))
    assert np.array_equal(L64.astype(np.float32), Oracle(logspec_cfg(case)).process(x))
    G = config_table(trap_cfg(case), "trap")
    assert G.shape == (ndct * traplen,) and np.abs(G.reshape(ndct, traplen).sum(axis=1)).max() < 1e-12   # rows sum to zero: the mean removal
    R64 = contract(G, L64, traplen, ndct)
    assert (np.abs(R64 - ref) <= 2.0 ** -24 * np.abs(ref) + 1e-10).all(), float(np.abs(R64 - ref).max())


@pytest.fixture(scope="module")
def conditioned():
    """Per case: the utterances, the oracle's rows, the float32 oracle log-mel rows and their float64 contraction."""
    out = {}
    for case in CASES:
        orc, lorc = Oracle(trap_cfg(case)), Oracle(logspec_cfg(case))
        G = config_table(trap_cfg(case), "trap")
        us = utterances(case)
        refs = [orc.process(u) for u in us]
        Ls = [lorc.process(u) for u in us]
        out[case] = (us, refs, Ls, [contract(G, L, case[2], case[3]) for L in Ls])
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_inputs_leave_the_kernel_half_of_the_bound(conditioned, case):
    """The float32-rounded oracle log-mel rows contracted in float64 lie within 0.5e-4 of the oracle's rows on every utterance of the
    GPU case: a condition on the cuts (tests/trap_cases.py: utterances), not a measurement of the engine."""
    us, refs, Ls, R64s = conditioned[case]
    counts = frame_counts(case[2])
    assert [r.shape[0] for r in refs] == counts and sum(counts) < 900 and counts.count(0) == 1
    worst = 0.0
    for ref, R64 in zip(refs, R64s):
        assert R64.shape == ref.shape and np.isfinite(ref).all()
        worst = max(worst, operation_error(R64, ref.astype(np.float64)))
    print("%s: float32 log-mel rows contracted in float64 against the oracle: %.3g" % (case_id(case), worst))
    assert worst <= 0.5 * TOL, worst


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("case", [SMALLEST, LARGEST], ids=case_id)
def test_the_comparator_sees_a_wrong_kernel(conditioned, case, fault):
    """A float32 rounding of the contraction passes assertion 2 of the GPU test on the case's own inputs; with a tap dropped (the first and
    the last, where the Hamming weight is smallest), the context shifted by a frame, the right clamp at T, a padded tap weighted or two
    bands swapped it fails, on every utterance with frames."""
    us, refs, Ls, R64s = conditioned[case]
    G = config_table(trap_cfg(case), "trap")
    for L, R64 in zip(Ls, R64s):
        if not L.shape[0]:
            continue
        assert operation_error(R64.astype(np.float32), R64) <= TOL
        wrong = contract(G, L, case[2], case[3], fault=fault).astype(np.float32)
        assert wrong.shape == R64.shape and operation_error(wrong, R64) > TOL, (fault, operation_error(wrong, R64))
