"""Offline TRAP-DCT (Engine.extract with -fea_kind trapdct) on both matrix-core kernels at the edges of their shape space
(tests/trap_cases.py: CASES), against two references:

  1. the oracle, to the project's parity bound (_assert_rows of tests/test_gpu_parity.py, 1e-4 of max(|oracle|, 1));
  2. the operation itself: the device's own float32 log-mel rows - the rows of an engine with -fea_kind logspec and otherwise the same
     options, run on the same list - contracted in numpy float64 with config_table(cfg, "trap"), to the same 1e-4 of max(|R64|, 1).  That
     holds the contraction alone to the tolerance, whatever the front end's share of it is.

The logspec rows are the plan's log-mel rows bit for bit by construction: the front end computes a band's logarithm once and stores it
either to the caller's rows (logspec) or to the plan's scratch (trapdct), from the same instruction stream (frontend_kernel.h: band_log,
band_to_scratch are run-time flags of one instantiation); the test asserts that both engines run the same instantiation (kernel_name)
and the same plan (the same list in one extract call each).

Every case is one extract call on a list whose utterances end and begin inside workgroup chunks of both kernels, with a frameless
utterance in the middle.  tests/test_trapdct_shapes_cpu.py holds what needs no GPU: the kernel path of every case, the LDS of every
accepted shape, the table against the reference's formula, the conditioning of these inputs, and that the comparator sees a wrong kernel.

Measured (MI355X), largest error of a case against the oracle / against the float64 contraction: DESIGN.md section 4.4."""
import numpy as np
import pytest

from ctucopy_amd import CtuError, config_table
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_gpu_parity import _assert_rows
from tests.trap_cases import CASES, SHIFT, TOL, WINDOW, case_id, contract, frame_counts, logspec_cfg, n_bands, operation_error, trap_cfg, utterances
from tests.util import C2, sig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_offline_trapdct_against_the_oracle_and_the_operation(Engine, case):
    path, bank, traplen, ndct = case
    cfg, lcfg = trap_cfg(case), logspec_cfg(case)
    assert tuple(int(v) for v in config_table(cfg, "trap_path")[:3]) == path
    B, counts = n_bands(bank), frame_counts(traplen)
    us = utterances(case)
    eng, leng = Engine(cfg), Engine(lcfg)
    assert eng.kernel_name() == leng.kernel_name()   # one front-end instantiation writes the log-mel rows of both
    got, Ls = eng.extract(us), leng.extract(us)
    G = config_table(cfg, "trap")
    orc = Oracle(cfg)
    e_oracle = e_op = e_in = 0.0
    fails = []
    for u, K, L, T in zip(us, got, Ls, counts):
        assert K.shape == (T, B * ndct) and K.dtype == np.float32 and L.shape == (T, B) and L.dtype == np.float32
        assert np.isfinite(K).all() and np.isfinite(L).all()
        ref = orc.process(u) if T else np.zeros((0, B * ndct), np.float32)
        assert ref.shape == K.shape
        R64 = contract(G, L, traplen, ndct)
        e_oracle = max(e_oracle, float((np.abs(K - ref) / np.maximum(np.abs(ref), 1.0)).max()) if T else 0.0)
        e_op = max(e_op, operation_error(K, R64))
        e_in = max(e_in, operation_error(R64, ref.astype(np.float64)))   # (no bound: what the log-mel rows alone bring to figure 1)
        try:
            _assert_rows(K, ref, cfg)
        except AssertionError as ex:
            fails.append(("oracle", T, str(ex)[:60]))
        if not (np.abs(K.astype(np.float64) - R64) <= TOL * np.maximum(np.abs(R64), 1.0)).all():
            fails.append(("operation", T, operation_error(K, R64)))
    print("TRAPDCT %s %s: against the oracle %.3e, against the float64 contraction of the device's log-mel rows %.3e (that contraction against the oracle: %.3e)"
          % (case_id(case), "split16" if path[0] else "mfma<%d,%d>" % path[1:], e_oracle, e_op, e_in))
    assert not fails, (e_oracle, e_op, fails)


def test_a_middle_utterance_of_half_a_context_is_refused(Engine):
    """plan.cc: trapdct on fewer than (traplen + 1) / 2 frames is undefined in the reference.  half frames in the middle of a batch refuse
    the batch, in the plan's words; half + 1 frames and a frameless utterance there are taken."""
    eng = Engine(C2 + ["-fea_kind", "trapdct,31,8"])
    half = 15
    n = lambda f: WINDOW - SHIFT + f * SHIFT
    assert [eng.num_frames(n(f)) for f in (half, half + 1)] == [half, half + 1]
    with pytest.raises(CtuError) as ei:
        eng.plan([n(half + 1), n(half), n(half + 1)])
    assert ei.value.code == ceng.CTU_ERR_INPUT and "trapdct on fewer than (traplen+1)/2 frames" in str(ei.value)
    x = sig("CS0")
    with pytest.raises(CtuError) as ei:
        eng.extract([x[:n(64)], x[:n(half)], x[:n(64)]])
    assert ei.value.code == ceng.CTU_ERR_INPUT and "trapdct on fewer than (traplen+1)/2 frames" in str(ei.value)
    for mid in (n(half + 1), 300):
        plan = eng.plan([n(half + 1), mid, n(half + 1)])
        assert plan.total_frames == 2 * (half + 1) + max(eng.num_frames(mid), 0)
        plan.close()
