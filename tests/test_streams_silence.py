"""Stream sets on digital silence (Engine.streams_ex): the first file of a case of tests/util.py's REF_E2E_SILENCE_CASES - speech around a
block of zeros, a muted telephone channel - pushed through a set gives what a fresh engine's offline run of the same file gives.  The
per-stream state carries the non-finite values the all-zero frames make from launch to launch: CMS mean, log-mel context, detector,
noise estimates, overlap-add tail; and the packed pairs of the 256-point transform and the eight-frame steps fall differently when a
file is cut into pushes.  One set per state flag, with the smallest chain that uses it, and two schedules each: pushes of eight hops, and
one that cuts twice inside the zero block at samples that are multiples of neither the hop nor 8, so that a push begins and ends on zeros.

The rule in every schedule: row counts and VAD bytes equal; a row is finite in one run exactly when it is in the other; the finite rows
bit-equal wherever the existing streamed test of that flag asserts bit identity (the eight-hop schedule; any chunking on the large
transforms), elsewhere under that test's own bound against the oracle.  The bits of non-finite values are not compared: no contract
fixes a NaN's payload.  The offline side is held to the compiled reference in tests/test_ref_e2e_silence_gpu.py."""
import numpy as np
import pytest

from ctucopy_amd import engine as ceng
from ctucopy_amd import streams_flags_for
from oracle.oracle import Oracle
from tests.test_gpu_parity import _assert_rows
from tests.test_streams_ss import _ss_rule
from tests.util import M44, REF_E2E_SILENCE_CASES, SIG_EXTEN, zeros_mid, zeros_mid_parts

pytestmark = pytest.mark.gpu

ROW, NR, VAD, SIGNAL, TRAP, SS, SS_LARGE = (ceng.STREAMS_ROW_STATE, ceng.STREAMS_NR_STATE, ceng.STREAMS_VAD_STATE, ceng.STREAMS_SIGNAL_STATE,
                                            ceng.STREAMS_TRAP_STATE, ceng.STREAMS_SS_STATE, ceng.STREAMS_SS_LARGE_STATE)
# name -> (command line, samples of zeros_mid, the flags the chain needs, bit identity on the eight-hop schedule, on any schedule)
SETS = {
    "row_state": REF_E2E_SILENCE_CASES["sil_da_zexp_e"] + (ROW, True, False),
    "nr_state": REF_E2E_SILENCE_CASES["sil_c4_novad"] + (NR, True, False),
    "nr_vad_state": REF_E2E_SILENCE_CASES["sil_c4"] + (NR | VAD, True, False),
    "vad_state": REF_E2E_SILENCE_CASES["sil_vad_energy_dyn"] + (VAD, True, False),
    # 23 bands: the offline run launches the 16-bit split kernel, the stream the fp32 one (tests/test_streams_trap.py holds C5 to the oracle bound)
    "trap_state": REF_E2E_SILENCE_CASES["sil_trapdct51"] + (TRAP, False, False),
    "ss_state": REF_E2E_SILENCE_CASES["sil_fwss"] + (SS, True, False),
    "signal_nr_state": (SIG_EXTEN, "sil12000", SIGNAL | NR, True, False),
    "ss_large_state": (M44 + "-nr_mode fwss -vad burg".split(), "sil23151", SS | SS_LARGE, True, True),     # 3 windows of 1102 samples + 45 shifts of 441
}


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


_CASE = {}


def _case(Engine, name):
    """(signal, what a fresh engine's offline run gives, what the oracle gives) of a set's chain: made once, shared by both schedules, never written."""
    if name not in _CASE:
        cfg, inp, flags = SETS[name][:3]
        x = zeros_mid(int(inp[len("sil"):]))
        x.setflags(write=False)
        fresh = Engine(cfg)      # zero noise seed, detector rebuilt
        if flags & SIGNAL:
            off, ref = (fresh.enhance([x])[0], None), (Oracle(cfg).enhance(x), None)
        elif flags & VAD:
            rows, vads = fresh.extract([x], want_vad=True)
            off, ref = (rows[0], np.asarray(vads[0])), Oracle(cfg).process(x, want_vad=True)
        else:
            off, ref = (fresh.extract([x])[0], None), (Oracle(cfg).process(x), None)
        for a in off + tuple(ref):
            if a is not None:
                a.setflags(write=False)
        _CASE[name] = (x, off, ref)
    return _CASE[name]


def _stream(st, sid, x, chunks, flags):
    """Pushes x in `chunks` on stream sid and finishes: (rows or samples, decisions or None)."""
    out, dec, at = [], [], 0
    for c in chunks + [None]:
        if flags & SIGNAL:
            r, v = (st.push_signal({sid: x[at:at + c]})[sid] if c is not None else st.finish_signal(sid)), None
        elif flags & VAD:
            r, v = st.push({sid: x[at:at + c]}, want_vad=True)[sid] if c is not None else st.finish(sid, want_vad=True)
        else:
            r, v = (st.push({sid: x[at:at + c]})[sid] if c is not None else st.finish(sid)), None
        at += c or 0
        out.append(r.copy())
        dec.append(None if v is None else v.copy())
    assert at == x.size and st.frames(sid) == 0 and st.pending(sid) == 0
    return np.concatenate(out), (np.concatenate(dec) if flags & VAD else None)


def _eights(eng, n):
    """A push that completes eight frames, pushes of eight hops, the rest."""
    w, s = eng.dims.window, eng.dims.wshift
    out = [w + 7 * s]
    while sum(out) + 8 * s <= n:
        out.append(8 * s)
    return out + [n - sum(out)]


def _cut_in_the_block(eng, n):
    """Four pushes: half the speech ahead of the block, up to a third of the way into the block, from zeros to zeros across its middle third,
    the rest.  The two cuts inside the block are multiples of neither the hop nor 8."""
    s = eng.dims.wshift
    a, z, _ = zeros_mid_parts(n)
    cuts = []
    for c in (a + z // 3, a + 2 * z // 3):
        while c % s == 0 or c % 8 == 0:
            c += 1
        cuts.append(c)
    assert a < cuts[0] < cuts[1] < a + z and all(c % s and c % 8 for c in cuts)
    at = [0, a // 2 + 3] + cuts + [n]
    return [q - p for p, q in zip(at[:-1], at[1:])]


def _finite(a):
    return np.isfinite(a).all(axis=1)


def _compare(name, tag, cfg, flags, identical, got, off, ref):
    (g, gv), (o, ov), (r, rv) = got, off, ref
    assert g.shape == o.shape and g.dtype == o.dtype, (name, tag, g.shape, o.shape)
    if flags & SIGNAL:
        d, do = np.abs(g.astype(int) - o.astype(int)), np.abs(g.astype(int) - r.astype(int))
        print(f"streams on silence {name}, {tag}: {g.size} samples, {int((d > 0).sum())} differ from the offline run, worst {int(d.max())} LSB; "
              f"against the oracle max {int(do.max())} LSB, mean {do.mean():.4f}")
        if identical:
            assert np.array_equal(g, o), (name, tag)
        else:    # tests/test_streams_signal.py: 1 LSB against the offline run, 2 LSB and a mean of 0.3 against the oracle behind exten
            assert d.max() <= 1 and r.shape == g.shape and do.max() <= 2 and do.mean() <= 0.3, (name, tag, int(d.max()), int(do.max()), float(do.mean()))
        return
    fg, fo = _finite(g), _finite(o)
    both = fg & fo
    diff = np.abs(g[both].astype(np.float64) - o[both]) / np.maximum(np.abs(o[both]), 1.0)
    print(f"streams on silence {name}, {tag}: {g.shape[0]} rows, non-finite streamed {np.flatnonzero(~fg).tolist()}, offline {np.flatnonzero(~fo).tolist()}; "
          f"finite rows: {int((g[both] != o[both]).any(axis=1).sum())} not bit-equal, largest |streamed - offline| / max(|offline|, 1) {float(diff.max()) if diff.size else 0.0:.3e}"
          + ("" if gv is None else f"; {gv.size} VAD bytes, differ at {np.flatnonzero(gv != ov).tolist() if gv.size == ov.size else None}, {int((ov == ord('1')).sum())} ones"))
    if gv is not None:
        assert np.array_equal(gv, ov), (name, tag)
        assert np.array_equal(ov, rv)                              # (the offline decisions are the oracle's, and hold both values)
        assert set(np.unique(ov)) == {ord("0"), ord("1")}
    assert (~fo).any() == (name not in ("ss_state", "ss_large_state")) and fo.sum() >= 20      # (fwss floors what it subtracts: finite on zeros)
    assert np.array_equal(fg, fo), (name, tag, np.flatnonzero(fg != fo).tolist())
    if identical:
        assert np.array_equal(g[fo], o[fo]), (name, tag)
        return
    assert r.shape == g.shape and np.isfinite(r[fo]).all(), (name, tag)
    if flags & SS:
        _ss_rule(g[fo], r[fo], cfg)
    else:
        _assert_rows(g[fo], r[fo], cfg)
        if flags & TRAP:
            _assert_rows(g[fo], o[fo], cfg)        # "to rounding": no further from the offline run than the oracle may be


@pytest.mark.parametrize("schedule", ["eight_hops", "cut_in_the_block"])
@pytest.mark.parametrize("name", list(SETS))
def test_a_file_with_a_zero_block_streams_as_it_runs_offline(Engine, name, schedule):
    cfg, inp, flags, eights_identical, any_identical = SETS[name]
    assert streams_flags_for(cfg)[:3] == (ceng.CTU_OK, flags, "")       # the smallest chain that needs exactly these flags
    x, off, ref = _case(Engine, name)
    eng = Engine(cfg)
    if schedule == "eight_hops":
        chunks, n_streams, sid, identical = _eights(eng, x.size), 2, 1, eights_identical
    else:
        chunks, n_streams, sid, identical = _cut_in_the_block(eng, x.size), 1, 0, any_identical
    st = eng.streams_ex(n_streams, max(chunks), flags)
    got = _stream(st, sid, x, chunks, flags)
    _compare(name, schedule, cfg, flags, identical, got, off, ref)
