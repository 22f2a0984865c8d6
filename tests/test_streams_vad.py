"""Stream sets with detector state on the GPU (Engine.streams(..., vad_state=True)): the VAD module behind pushed samples gives the
decisions and rows of the offline run, a frame's row leaving with its decision h = (vad_filter_order - 1) / 2 frames late, with the
detector's state (thresholds, background cepstrum, the majority filter's ring) kept per stream between the pushes.

Every test first holds the offline decisions to the oracle's and asks that they contain both values (hence a transition): a detector
that never fires would pass everything below.

Bounds.  Decisions: equality, the suite's standing bar for offline runs - against the offline run and against the oracle, under every
chunking.  Rows: bit identity against the offline run where DESIGN.md section 4.10 derives it for the front end - every chunking at
512 points, and at 256 points (two frames share a complex transform) pushes that complete an even number of frames, which keep every
frame's partner; where a push of an odd number of frames changes the partner (256 points: C4) the oracle bound of
tests/test_gpu_parity.py (_assert_rows), imported, as tests/test_streams.py and tests/test_streams_nr.py hold such chunkings."""
import numpy as np
import pytest

from ctucopy_amd import CtuError, streams_vad_step
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_gpu_parity import _assert_rows
from tests.test_streams import _schedule, _signal
from tests.util import C2, C4, _swap, sig

pytestmark = pytest.mark.gpu

BURG = "-vad burg -vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode lpc".split()
ENERGY = "-vad_out_mode vad -vad_cri_mode energy".split()
CONFIGS = [C4, _swap(C4, "-vad_thr_mode", "dyn"), C4 + ["-vad_filter_order", "7"], C2 + BURG + ["-vad_thr_mode", "adapt"],
           C2 + ["-w", "20"] + BURG + ["-vad_thr_mode", "dyn"], C2 + ENERGY + ["-vad_thr_mode", "dyn"],
           C2 + ENERGY + ["-vad_thr_mode", "perc", "-vad_filter_order", "5"],
           _swap(C4, "-vad_thr_mode", "perc"), _swap(C4, "-vad_thr_mode", "absolute") + ["-vad_absolute_thr", "5"]]
IDS = ["c4_adapt", "c4_dyn", "c4_order7", "mfcc_burg_adapt_fused512", "mfcc_w20_burg_dyn", "mfcc_energy_dyn", "mfcc_energy_perc_order5",
       "c4_perc", "c4_absolute5"]


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def _order(cfg):
    return int(cfg[cfg.index("-vad_filter_order") + 1]) if "-vad_filter_order" in cfg else 3


def _set(eng, cfg, n, max_push):
    return eng.streams(n, max_push, nr_state="exten" in cfg, vad_state=True)


_ORACLE = {}


def _offline(eng, cfg, x, both=True):
    """(rows, decisions, the oracle's rows) of the offline run, after holding the decisions to the oracle's (computed once per
    configuration and signal) and, with `both`, to containing both values and a transition."""
    key = (tuple(cfg), x.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = Oracle(cfg).process(x, want_vad=True)
    ref_rows, ref_vad = _ORACLE[key]
    rows, vads = eng.extract([x], want_vad=True)
    off, vad = rows[0], vads[0]
    assert off.shape == ref_rows.shape and vad.shape == ref_vad.shape == (off.shape[0],)
    assert np.array_equal(vad, ref_vad), np.nonzero(vad != ref_vad)[0][:8]
    if both:
        assert set(np.unique(vad)) == {ord("0"), ord("1")} and np.count_nonzero(np.diff(vad.astype(np.int16))) >= 1
    return off, vad, ref_rows


def _stream(eng, st, sid, x, chunks, cfg):
    """Pushes x in `chunks` on stream sid and finishes: (rows, decisions), after checking every push's count, st.frames and st.pending
    against R(F), and that finish delivers the h frames held back."""
    order, w, s = _order(cfg), eng.dims.window, eng.dims.wshift
    h = (order - 1) // 2
    rows, vads, at = [], [], 0
    for c in chunks:
        r, v = st.push({sid: x[at:at + c]}, want_vad=True)[sid]
        at += c
        rows.append(r)
        vads.append(v)
        out, pending = streams_vad_step(w, s, order, at)
        F = max(eng.num_frames(at), 0)
        assert out + pending == F and out == (F - h if F > h else 0)
        assert r.shape[0] == v.shape[0] and sum(g.shape[0] for g in rows) == out == st.frames(sid) and st.pending(sid) == pending, (at, c)
    F = max(eng.num_frames(at), 0)
    r, v = st.finish(sid, want_vad=True)
    assert r.shape[0] == v.shape[0] == (h if F > h else 0) and st.frames(sid) == 0 and st.pending(sid) == 0
    rows.append(r)
    vads.append(v)
    return np.concatenate(rows), np.concatenate(vads)


def _eights(eng, x, first=8):
    """A push that completes `first` frames, pushes of eight hops, the rest."""
    w, s = eng.dims.window, eng.dims.wshift
    out = [w + (first - 1) * s] if first else [w - 1]
    while sum(out) + 8 * s <= x.size:
        out.append(8 * s)
    return out + [x.size - sum(out)]


def _rows_identical(eng, chunks):
    """Whether section 4.10 derives bit identity of the rows for this chunking: always at 512 points; at 256 points while every push
    completes an even number of frames."""
    if eng.dims.wfft != 256:
        return True
    at, frames = 0, []
    for c in chunks:
        at += c
        frames.append(max(eng.num_frames(at), 0))
    return all((b - a) % 2 == 0 for a, b in zip([0] + frames[:-1], frames))


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_pushes_of_eight_hops_give_the_offline_rows_and_decisions(Engine, cfg):
    eng = Engine(cfg)
    x = _signal(eng, 96)
    off, vad, _ = _offline(eng, cfg, x)
    assert off.shape[0] == 96
    st = _set(eng, cfg, 2, eng.dims.window + 8 * eng.dims.wshift)
    rows, dec = _stream(eng, st, 1, x, _eights(eng, x), cfg)
    assert dec.shape == vad.shape and np.array_equal(dec, vad), np.nonzero(dec != vad)[0][:8]
    assert rows.shape == off.shape and np.array_equal(rows, off)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_the_detector_s_init_segments_cross_pushes(Engine, cfg):
    """t == 0 and t == 1 in different launches; a first push of 72 frames (two tiles) and pushes that load the state behind it; a first
    push of h frames, which delivers nothing.  Largest |streamed - offline| / max(|offline|, 1) of the rows where a push of an odd
    number of frames changes a frame's partner at 256 points: printed, and in DESIGN.md section 4.10 (Detector state)."""
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    h = (_order(cfg) - 1) // 2
    x = _signal(eng, 96)
    off, vad, ref = _offline(eng, cfg, x)
    one_by_one = [w, s] + [8 * s] * 11
    one_by_one.append(x.size - sum(one_by_one))
    held = _eights(eng, x, first=h)
    for name, chunks in (("one frame, one frame, eight hops", one_by_one), ("72 frames, eight hops", _eights(eng, x, first=72)), ("h frames, eight hops", held)):
        st = _set(eng, cfg, 1, max(chunks))
        if chunks is held:
            assert max(eng.num_frames(chunks[0]), 0) == h   # (the helper holds the push to R(h) = 0 rows and h frames pending)
        rows, dec = _stream(eng, st, 0, x, chunks, cfg)
        assert dec.shape == vad.shape and np.array_equal(dec, vad), (name, np.nonzero(dec != vad)[0][:8])
        assert rows.shape == off.shape
        if _rows_identical(eng, chunks):
            assert np.array_equal(rows, off), name
        else:
            print(name, "- streamed vs offline rows, largest |difference| / max(|offline|, 1):",
                  float((np.abs(rows - off) / np.maximum(np.abs(off), 1.0)).max()), " ".join(cfg))
            _assert_rows(rows, ref, cfg)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_arbitrary_chunking_gives_the_oracle_s_decisions(Engine, cfg):
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 96)
    off, vad, ref = _offline(eng, cfg, x)
    st = _set(eng, cfg, 1, max(w, 17 * s))
    rows, dec = _stream(eng, st, 0, x, _schedule(eng, x.size, 11), cfg)
    assert dec.shape == vad.shape and np.array_equal(dec, vad), np.nonzero(dec != vad)[0][:8]
    assert rows.shape == ref.shape and np.isfinite(rows).all()
    print("streamed vs offline rows, largest |difference| / max(|offline|, 1):", float((np.abs(rows - off) / np.maximum(np.abs(off), 1.0)).max()), " ".join(cfg))
    _assert_rows(rows, ref, cfg)


def test_c4_at_16_khz_runs_the_512_point_fused_front_end_with_both_states(Engine):
    """exten ahead of the fused detector at 512 points: the second of the two frontend_kernel<..., VF, XS> instantiations (C4 itself, at
    8 kHz, runs the 256-point one).  The decisions are held to the offline run's and the oracle's; whether they hold both values on this
    signal is not asked of this configuration (the seven above are the ones probed for it)."""
    cfg = C2 + ["-nr_mode", "exten", "-nr_a", "2"] + BURG + ["-vad_thr_mode", "adapt"]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    assert eng.dims.wfft == 512 and "VF" in eng.kernel_name() and "exten" in eng.kernel_name()
    x = _signal(eng, 96)
    off, vad, ref = _offline(eng, cfg, x, both=False)
    rows, dec = _stream(eng, _set(eng, cfg, 2, w + 8 * s), 1, x, _eights(eng, x), cfg)
    assert np.array_equal(dec, vad) and np.array_equal(rows, off)
    rows, dec = _stream(eng, _set(eng, cfg, 1, max(w, 17 * s)), 0, x, _schedule(eng, x.size, 11), cfg)
    assert np.array_equal(dec, vad), np.nonzero(dec != vad)[0][:8]
    _assert_rows(rows, ref, cfg)


def test_a_file_of_three_frames_at_order_seven_writes_nothing_and_the_next_file_is_a_fresh_one(Engine):
    cfg = C4 + ["-vad_filter_order", "7"]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x, y = _signal(eng, 40, seed=9), _signal(eng, 96)   # (the second file is the signal whose decisions hold both values)
    offy, vady, _ = _offline(eng, cfg, y)
    fresh = _stream(eng, _set(eng, cfg, 2, w + 8 * s), 1, y, _eights(eng, y), cfg)
    st = _set(eng, cfg, 2, w + 8 * s)
    r, v = st.push({1: x[:w + 2 * s]}, want_vad=True)[1]   # three frames: no more than the filter delays
    assert eng.num_frames(w + 2 * s) == 3 and r.shape[0] == v.shape[0] == 0 and st.frames(1) == 0 and st.pending(1) == 3
    r, v = st.finish(1, want_vad=True)   # CTU_OK, nothing written: the reference writes nothing for such a file
    assert r.shape == (0, eng.dims.row_floats) and v.shape == (0,) and st.pending(1) == 0
    again = _stream(eng, st, 1, y, _eights(eng, y), cfg)
    assert np.array_equal(again[1], fresh[1]) and np.array_equal(again[0], fresh[0])
    assert np.array_equal(again[1], vady) and np.array_equal(again[0], offy)


@pytest.mark.parametrize("cfg", [C4, C2 + ENERGY + ["-vad_thr_mode", "perc", "-vad_filter_order", "5"]], ids=["c4_adapt", "mfcc_energy_perc_order5"])
def test_thirty_seven_streams_in_different_phases_share_a_push(Engine, cfg):
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    n = _signal(eng, 96).size
    base = sig("CS0") if eng.dims.fs == 16000 else None
    xs = [_signal(eng, 96)] + [base[k * 9001:k * 9001 + n].copy() if base is not None else _signal(eng, 96, seed=50 + k) for k in range(1, 5)]
    assert len({x.tobytes() for x in xs}) == 5
    offl = [_offline(eng, cfg, x, both=k == 0)[:2] for k, x in enumerate(xs[:4])]   # (A's file is the signal every other test here runs)
    N, A, B, C, D = 37, 5, 0, 2, 1   # A starts a file in the push, B goes on, C completes no frame, D is in its second file
    of = {k: k % 3 for k in range(N)}   # the signal of every stream: 0 .. 2, and 3 for D's second file
    of[A], of[B], of[C] = 0, 1, 2
    alone_a = _stream(eng, _set(eng, cfg, 1, w + 8 * s), 0, xs[0], _eights(eng, xs[0]), cfg)
    fresh_d = _stream(eng, _set(eng, cfg, 1, w + 8 * s), 0, xs[3], _eights(eng, xs[3]), cfg)
    st = _set(eng, cfg, N, w + 8 * s)
    got = {k: ([], []) for k in range(N)}

    def take(out):
        for k, (r, v) in out.items():
            got[k][0].append(r)
            got[k][1].append(v)

    # ahead of the push in question: every stream but A and D has had a first push, D a whole file
    take(st.push({k: xs[of[k]][:w + 7 * s] for k in range(N) if k not in (A, D)}, want_vad=True))
    first_d = _stream(eng, st, D, xs[4], _eights(eng, xs[4]), cfg)
    assert first_d[0].shape[0] == first_d[1].shape[0] == 96
    of[D] = 3
    at = {k: (0 if k in (A, D) else w + 7 * s) for k in range(N)}
    step = {k: (w + 7 * s if k in (A, D) else s // 2 if k == C else 8 * s) for k in range(N)}
    h = (_order(cfg) - 1) // 2
    out = st.push({k: xs[of[k]][at[k]:at[k] + step[k]] for k in range(N)}, want_vad=True)   # the push: all 37
    assert [out[k][0].shape[0] for k in (A, B, C, D)] == [8 - h, 8, 0, 8 - h]
    take(out)
    for k in range(N):
        at[k] += step[k]
    while any(at[k] < n for k in range(N)):
        p = {k: xs[of[k]][at[k]:at[k] + 8 * s] for k in range(N) if at[k] < n}
        take(st.push(p, want_vad=True))
        for k in p:
            at[k] += p[k].size
    wrong = []
    for k in range(N):
        assert st.frames(k) == 96 - h
        r, v = st.finish(k, want_vad=True)
        rows, dec = np.concatenate(got[k][0] + [r]), np.concatenate(got[k][1] + [v])
        if not (np.array_equal(dec, offl[of[k]][1]) and np.array_equal(rows, offl[of[k]][0])):
            wrong.append(k)
        if k == A:
            assert np.array_equal(dec, alone_a[1]) and np.array_equal(rows, alone_a[0])
        if k == D:
            assert np.array_equal(dec, fresh_d[1]) and np.array_equal(rows, fresh_d[0])
    assert not wrong, wrong


def test_calls_on_the_wrong_kind_of_set(Engine):
    cfg = C2 + ENERGY + ["-vad_thr_mode", "dyn"]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 40)
    chunks = _eights(eng, x)
    with_vad = _stream(eng, _set(eng, cfg, 1, w + 8 * s), 0, x, chunks, cfg)
    # the old push and finish on a set with detector state: the same rows, the decisions stay behind
    st = _set(eng, cfg, 1, w + 8 * s)
    rows, at = [], 0
    for c in chunks:
        rows.append(st.push({0: x[at:at + c]})[0])
        at += c
    rows.append(st.finish(0))
    assert rows[-1].shape[0] == 1 and np.array_equal(np.concatenate(rows), with_vad[0])
    # decisions asked of a set without detector state: CTU_ERR_INPUT before anything changes
    with pytest.raises(CtuError) as ei:
        eng.streams(1, w + 8 * s)
    assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and "VAD module" in str(ei.value)
    plain = Engine(C2)
    for kw in ({}, {"vad_state": True}):   # (on a configuration without the VAD module the flag changes nothing)
        ps = plain.streams(1, w + 8 * s, **kw)
        with pytest.raises(CtuError) as ei:
            ps.push({0: x[:chunks[0]]}, want_vad=True)
        assert ei.value.code == ceng.CTU_ERR_INPUT and "detector state" in str(ei.value)
        assert ps.frames(0) == 0
        first = ps.push({0: x[:chunks[0]]})[0]
        assert first.shape[0] == 8 and np.array_equal(first, plain.extract([x])[0][:8])
        with pytest.raises(CtuError) as ei:
            ps.finish(0, want_vad=True)
        assert ei.value.code == ceng.CTU_ERR_INPUT and ps.frames(0) == 8
        assert ps.finish(0).shape[0] == 0 and ps.frames(0) == 0


def test_a_refused_signal_call_between_pushes_with_decisions_changes_nothing(Engine):
    """Turn and descriptor reuse across call kinds on one set, the mirror of tests/test_streams_signal.py's: pushes of one to three hops
    on a set of three streams with detector state (512 points: every chunking gives the offline rows bit for bit), a finish between two
    pushes, and a signal call, which is refused and must leave the turn, the push counter and the mirrors alone."""
    cfg = C2 + BURG + ["-vad_thr_mode", "adapt"]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    assert eng.dims.wfft == 512
    hops = {0: [3, 0, 1, 2, 0, 3], 1: [0, 2, 3, 0, 1, 2], 2: [0, 3, 0, 2, 1, 3]}   # per push (stream 1: its second file)
    lead = w - s                                                                  # (behind it a push of k hops completes k frames)
    first1 = _signal(eng, 4)[:lead + 3 * s].copy()                                # stream 1's first file: three frames
    xs = {k: _signal(eng, 40)[100 * k:100 * k + lead + sum(hops[k]) * s].copy() for k in hops}
    st = _set(eng, cfg, 3, lead + 3 * s)
    rows, vads, at = {k: [] for k in hops}, {k: [] for k in hops}, {k: 0 for k in hops}

    def take(out):
        for k, (r, v) in out.items():
            rows[k].append(r.copy())
            vads[k].append(v.copy())

    def push(i):
        p = {k: xs[k][at[k]:at[k] + hops[k][i] * s + (0 if at[k] else lead)] for k in hops if hops[k][i]}
        take(st.push(p, want_vad=True))
        for k in p:
            at[k] += p[k].size

    out = st.push({0: xs[0][:lead + 3 * s], 1: first1}, want_vad=True)
    take({0: out[0]})
    at[0] = lead + 3 * s
    fin = st.finish(1, want_vad=True)
    file1 = (np.concatenate([out[1][0], fin[0]]), np.concatenate([out[1][1], fin[1]]))
    assert st.frames(1) == 0 and st.pending(1) == 0
    push(1)                                                  # streams 1 and 2: stream 1 starts its second file
    before = [(st.frames(k), st.pending(k)) for k in hops]
    with pytest.raises(CtuError) as ei:
        st.push_signal({0: xs[0][at[0]:at[0] + s]})
    assert ei.value.code == ceng.CTU_ERR_INPUT
    assert "ctu_streams_push_signal / ctu_streams_finish_signal need a set with signal state" in str(ei.value)
    assert [(st.frames(k), st.pending(k)) for k in hops] == before
    for i in range(2, 6):                                    # four more
        push(i)
    off1, vad1, _ = _offline(eng, cfg, first1, both=False)
    assert np.array_equal(file1[0], off1) and np.array_equal(file1[1], vad1)
    for k in hops:
        assert at[k] == xs[k].size
        take({k: st.finish(k, want_vad=True)})
        off, vad, _ = _offline(eng, cfg, xs[k], both=False)
        assert off.shape[0] == sum(hops[k])
        assert np.array_equal(np.concatenate(vads[k]), vad), k
        assert np.array_equal(np.concatenate(rows[k]), off), k
