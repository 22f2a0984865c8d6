"""Stream sets with detector state behind row state on the GPU (Engine.streams_ex(..., STREAMS_ROW_STATE | STREAMS_VAD_STATE |
STREAMS_VAD_ROW_STATE)):
the VAD module with a delta chain, a stacking or CMS behind it gives the decisions and rows of the offline run.  The detector is called
when a chain row is complete - call j, by its own index, on the criterion of frame min(j + delay, T - 1) - and a row leaves with its
decision h = (vad_filter_order - 1) / 2 calls later, or with finish, which makes the calls the file still owes on its last frame.

Every test first holds the offline decisions to the oracle's and (on the 96-frame signal) asks that they contain both values: a detector
that never fires would pass everything below.  The configurations and the oracle's side of these premises: tests/test_streams_vad_rows_cpu.py.

Bounds (none is new).  Decisions: equality, against the offline run and against the oracle, under every chunking.  Rows: bit identity
against the offline run where tests/test_streams_rows.py and tests/test_streams_vad.py derive it - pushes that end a multiple of eight
frames into the file (an even number of frames per push at 256 points), delta windows of 2, block 0, stacking and both CMS forms - and
elsewhere the oracle bound of tests/test_gpu_parity.py (_assert_rows), imported."""
import numpy as np
import pytest

from ctucopy_amd import CtuError, streams_vad_rows_step
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_gpu_parity import _assert_rows
from tests.test_streams import _schedule, _signal
from tests.test_streams_vad_rows_cpu import C4_ZEXP, CONFIGS, NR, THREE, TODAY_DELTA
from tests.util import sig

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


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


def _stream(eng, st, sid, x, chunks, shape):
    """Pushes x in `chunks` on stream sid and finishes: (rows, decisions), after checking every push's count, st.frames and st.pending
    against ctu_streams_vad_rows_step, and that finish delivers exactly what is pending (nothing from a file of no more than h frames)."""
    delay, wmax, h = shape
    order, w, s = 2 * h + 1, eng.dims.window, eng.dims.wshift
    rows, vads, at = [], [], 0
    for c in chunks:
        r, v = st.push({sid: x[at:at + c]}, want_vad=True)[sid]
        at += c
        rows.append(r)
        vads.append(v)
        out, pending = streams_vad_rows_step(w, s, order, delay, wmax, at)
        F = max(eng.num_frames(at), 0)
        calls = F if delay == 0 else (max(F - delay, 0) if F >= wmax + 2 else 0)
        assert out + pending == F and out == max(calls - h, 0)
        assert r.shape[0] == v.shape[0] and sum(g.shape[0] for g in rows) == out == st.frames(sid) and st.pending(sid) == pending, (at, c)
    F = max(eng.num_frames(at), 0)
    pending = st.pending(sid)
    r, v = st.finish(sid, want_vad=True)
    assert r.shape[0] == v.shape[0] == (pending if F > h else 0) and st.frames(sid) == 0 and st.pending(sid) == 0
    rows.append(r)
    vads.append(v)
    return np.concatenate(rows), np.concatenate(vads)


def _eights(eng, x, first=8):
    """A push that completes `first` frames, pushes of eight hops, the rest."""
    w, s = eng.dims.window, eng.dims.wshift
    out = [w + (first - 1) * s]
    while sum(out) + 8 * s <= x.size:
        out.append(8 * s)
    return out + [x.size - sum(out)]


def _firsts(eng, x, frames, then=8):
    """Pushes whose ends complete `frames` (ascending frame counts of the file), pushes of `then` hops behind them, the rest."""
    w, s = eng.dims.window, eng.dims.wshift
    out, done = [], 0
    for f in frames:
        out.append((w if done == 0 else 0) + (f - max(done, 1)) * s)
        done = f
    while sum(out) + then * s <= x.size:
        out.append(then * s)
    return out + [x.size - sum(out)]


def _bit_identical(eng, chunks):
    """Whether the rows of this chunking are the offline run's bit for bit (tests/test_streams_rows.py: every push ends a multiple of
    eight frames into the file; the last may end anywhere: nothing follows it)."""
    at, ends = 0, []
    for c in chunks:
        at += c
        ends.append(max(eng.num_frames(at), 0))
    return all(f % 8 == 0 for f in ends[:-1])


def _check(eng, cfg, shape, x, chunks, off, vad, ref, name=""):
    st = eng.streams_ex(2, max(max(chunks), 1), THREE)
    rows, dec = _stream(eng, st, 1, x, chunks, shape)
    assert dec.shape == vad.shape and np.array_equal(dec, vad), (name, np.nonzero(dec != vad)[0][:8])
    assert rows.shape == off.shape
    if _bit_identical(eng, chunks):
        assert np.array_equal(rows, off), name
    else:
        print(name, "- streamed vs offline rows, largest |difference| / max(|offline|, 1):",
              float((np.abs(rows - off) / np.maximum(np.abs(off), 1.0)).max()) if off.size else 0.0, " ".join(cfg))
        _assert_rows(rows, ref, cfg)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_pushes_of_eight_hops_give_the_offline_rows_and_decisions(Engine, name):
    cfg, *shape = CONFIGS[name]
    eng = Engine(cfg)
    x = _signal(eng, 96)
    off, vad, _ = _offline(eng, cfg, x)
    assert off.shape[0] == 96
    st = eng.streams_ex(2, eng.dims.window + 8 * eng.dims.wshift, THREE)
    rows, dec = _stream(eng, st, 1, x, _eights(eng, x), shape)
    assert dec.shape == vad.shape and np.array_equal(dec, vad), np.nonzero(dec != vad)[0][:8]
    assert rows.shape == off.shape and np.array_equal(rows, off)


@pytest.mark.parametrize("name", ["energy_dyn_d_a", "energy_perc_o7_d_a_t", "energy_dyn_trap9"])
def test_the_edges_of_the_delay(Engine, name):
    """The first calls and the first rows in pushes of their own; a call per push; arbitrary pushes; and behind a stacking, whose halo is
    its largest window, the push in which the first calls are made with call 0's frame already behind it (the stream's record)."""
    cfg, *shape = CONFIGS[name]
    delay, wmax, h = shape
    eng = Engine(cfg)
    s = eng.dims.wshift
    x = _signal(eng, 96)
    off, vad, ref = _offline(eng, cfg, x)
    cases = [("delay, +1, +h, +h+1", _firsts(eng, x, sorted({delay, delay + 1, delay + h, delay + h + 1}))),
             ("one frame per push", _firsts(eng, x, list(range(1, 13)))),
             ("schedule 11", _schedule(eng, x.size, 11)), ("schedule 12", _schedule(eng, x.size, 12))]
    if name == "energy_dyn_trap9":
        assert delay == wmax == 4
        cases.append(("wmax + 1 frames, then one", _firsts(eng, x, [wmax + 1, wmax + 2])))
    for case, chunks in cases:
        assert sum(chunks) == x.size and min(chunks) >= 0
        _check(eng, cfg, shape, x, chunks, off, vad, ref, case)
    assert max(eng.num_frames(cases[0][1][0]), 0) == delay and cases[1][1][1] == s


@pytest.mark.parametrize("name, frames, index", [("energy_dyn_d_a", 72, 70), ("burg_adapt_d_a", 72, 70), ("energy_perc_o7_d_a_t", 72, 70),
                                                  ("energy_dyn_d_a", 12, 11), ("energy_perc_o7_d_a_t", 12, 11)])
def test_the_end_of_a_file_matters(Engine, name, frames, index):
    """A file cut from the 96-frame one ends in other decisions than the longer file has there: the calls of its last rows read its own
    last frame.  A stream learns the end at finish."""
    cfg, *shape = CONFIGS[name]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    whole = _signal(eng, 96)
    _, vad96, _ = _offline(eng, cfg, whole)
    x = whole[:w + (frames - 1) * s + s // 2].copy()
    off, vad, ref = _offline(eng, cfg, x, both=False)
    assert vad.size == frames and vad[index] != vad96[index]
    last_one = [w - 1, 1 + (frames - 2) * s]
    last_one.append(x.size - sum(last_one))
    assert eng.num_frames(sum(last_one[:2])) == frames - 1
    for case, chunks in (("eight hops", _eights(eng, x)), ("the last push completes one frame", last_one)):
        _check(eng, cfg, shape, x, chunks, off, vad, ref, case)


@pytest.mark.parametrize("name", ["energy_dyn_d_a", "energy_perc_o7_d_a_t"])
def test_short_files(Engine, name):
    """Files around h, the delay and the chain's shortest: the stream gives what a fresh run of the file gives - the same rows and bytes,
    or nothing - and where the offline plan refuses the file, finish refuses it in the same words and the stream takes a next file."""
    cfg, *shape = CONFIGS[name]
    delay, wmax, h = shape
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    whole = _signal(eng, 96)
    st = eng.streams_ex(1, w + (delay + h + 1) * s, THREE)
    for T in sorted({1, 2, 3, h, h + 1, delay, delay + 1, delay + h + 1} - {0}):
        x = whole[:w + (T - 1) * s + s // 2].copy()
        one_by_one = [w] + [s] * (T - 1) + [s // 2]
        assert sum(one_by_one) == x.size and eng.num_frames(x.size) == T
        if T < wmax + 2:   # the offline plan refuses the file (the oracle calls it undefined)
            with pytest.raises(CtuError) as ei:
                eng.extract([x], want_vad=True)
            assert "fewer than window+2 frames" in str(ei.value)
            off = None
        else:
            off, vad, ref = _offline(eng, cfg, x, both=False)
        for chunks in ([x.size], one_by_one):
            if off is None:
                at = 0
                for c in chunks:
                    r, v = st.push({0: x[at:at + c]}, want_vad=True)[0]
                    at += c
                    assert r.shape[0] == v.shape[0] == 0
                assert st.frames(0) == 0 and st.pending(0) == T
                with pytest.raises(CtuError) as ei:
                    st.finish(0, want_vad=True)
                assert ei.value.code == ceng.CTU_ERR_INPUT and "fewer than window+2 frames" in str(ei.value)
                assert st.frames(0) == 0 and st.pending(0) == 0
                continue
            rows, dec = _stream(eng, st, 0, x, chunks, shape)
            assert off.shape[0] == (T if T > h else 0)
            assert dec.shape == vad.shape and np.array_equal(dec, vad), (T, chunks, dec, vad)
            assert rows.shape == off.shape
            if off.size:
                _assert_rows(rows, ref, cfg)


@pytest.mark.parametrize("name", ["burg_adapt_d_a", "energy_perc_o7_d_a_t"])
def test_three_streams_keep_their_state_and_their_files_apart(Engine, name):
    cfg, *shape = CONFIGS[name]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    lead = w - s   # (behind it a push of k hops completes k frames)
    # hops per push, 0: the stream is not named in the push; stream 1 finishes a file of eleven frames behind push 3 and starts another
    hops = {0: [3, 0, 1, 2, 0, 3, 9, 8, 0, 5], 1: [4, 2, 5, 0, 1, 2, 3, 0, 8, 9], 2: [0, 5, 0, 2, 1, 3, 8, 8, 7, 0]}
    base = sig("CS0")
    first1 = base[7000:7000 + lead + 11 * s + 9].copy()
    xs = {0: base[:lead + sum(hops[0]) * s + 5].copy(), 1: base[3000:3000 + lead + sum(hops[1][3:]) * s + 7].copy(),
          2: base[9001:9001 + lead + sum(hops[2]) * s].copy()}
    src = {0: xs[0], 1: first1, 2: xs[2]}
    st = eng.streams_ex(3, lead + 9 * s + 9, THREE)
    got = {k: ([], []) for k in hops}
    at = {k: 0 for k in hops}

    def take(out):
        for k, (r, v) in out.items():
            got[k][0].append(r.copy())
            got[k][1].append(v.copy())

    for i in range(10):
        if i == 3:   # stream 1: the end of its first file (the samples left over complete no frame), and the second one begins
            take(st.push({1: src[1][at[1]:]}, want_vad=True))
            take({1: st.finish(1, want_vad=True)})
            file1 = (np.concatenate(got[1][0]), np.concatenate(got[1][1]))
            got[1] = ([], [])
            src[1], at[1] = xs[1], 0
            assert st.frames(1) == 0 and st.pending(1) == 0
        p = {k: src[k][at[k]:at[k] + hops[k][i] * s + (0 if at[k] else lead)] for k in hops if hops[k][i]}
        assert len(p) >= 2 or i == 3
        take(st.push(p, want_vad=True))
        for k in p:
            at[k] += p[k].size
    for k in hops:
        take(st.push({k: src[k][at[k]:]}, want_vad=True))
        take({k: st.finish(k, want_vad=True)})
    for k, x, (rows, dec) in [(1, first1, file1)] + [(k, xs[k], (np.concatenate(got[k][0]), np.concatenate(got[k][1]))) for k in hops]:
        off, vad, ref = _offline(eng, cfg, x, both=False)
        assert off.shape[0] == (11 if x is first1 else sum(hops[k][3:] if k == 1 else hops[k]))
        assert dec.shape == vad.shape and np.array_equal(dec, vad), (k, np.nonzero(dec != vad)[0][:8])
        assert rows.shape == off.shape
        _assert_rows(rows, ref, cfg)


def test_the_flags_on_the_device(Engine):
    cfg = CONFIGS["energy_dyn_d_a"][0]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    with pytest.raises(CtuError) as ei:
        eng.streams(1, w + 8 * s, row_state=True, vad_state=True)
    assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and TODAY_DELTA in str(ei.value)
    V = ceng.STREAMS_VAD_ROW_STATE
    for flags in (V, V | ceng.STREAMS_ROW_STATE, V | ceng.STREAMS_VAD_STATE):
        with pytest.raises(CtuError) as ei:
            eng.streams_ex(1, w + 8 * s, flags)
        assert ei.value.code == ceng.CTU_ERR_INPUT and "unknown stream set flags" in str(ei.value)
    assert eng.streams_ex(1, w + 8 * s, THREE).pending(0) == 0


def test_c4_with_cms_behind_the_fused_detector_and_the_noise_state(Engine):
    """exten ahead of the fused detector (delay 0: a call per frame, stream_vad_lanes_kernel as it stands) with exponential CMS behind
    it: rows through the row kernels, h = 1 behind their calls.  Eight-hop pushes, held as tests/test_streams_vad.py holds C4 to them."""
    cfg = C4_ZEXP
    eng = Engine(cfg)
    x = _signal(eng, 96)
    off, vad, _ = _offline(eng, cfg, x)
    st = eng.streams_ex(2, eng.dims.window + 8 * eng.dims.wshift, THREE | NR)
    rows, dec = _stream(eng, st, 1, x, _eights(eng, x), (0, 0, 1))
    assert dec.shape == vad.shape and np.array_equal(dec, vad), np.nonzero(dec != vad)[0][:8]
    assert rows.shape == off.shape and np.array_equal(rows, off)
