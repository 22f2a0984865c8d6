"""Stream sets with signal state on the GPU (Engine.streams(..., signal_state=True)): the speech-enhancement output behind pushed
samples is the offline run's (Engine.enhance), with the overlap-add's tail - and behind -nr_mode exten the noise estimate - kept per
stream between the pushes.

Bounds.  Bit identity where DESIGN.md section 4.10 derives it: pushes that end a multiple of eight frames into the file run the
front end's instruction stream over the same eight-frame steps, so the time-domain frames are the offline run's, and a sample's
partial sum continued in frame order is the offline run's sequence of additions.  Any other chunking moves the front end's last-bit
rounding, orders below 1.0 in the double sum ahead of floor(): a sample can cross an integer, not pass the next
one - 1 LSB against the offline run.  Against the oracle the bounds tests/test_gpu_parity.py::test_enhancement_output holds the
offline run to for the same configurations: 1 LSB and a mean of 0.05 for the plain chains, 2 LSB and 0.3 behind exten."""
import ctypes

import numpy as np
import pytest

from ctucopy_amd import CtuError, streams_signal_step
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_streams import _schedule, _signal

pytestmark = pytest.mark.gpu

SIG = "-fs 16000 -format_in raw -format_out raw".split()
PLAIN = ["-nr_mode", "none", "-fea_kind", "none", "-fb_definition", "none"]
CFG = {
    "A": SIG + ["-preset", "exten"],                                             # 512 / 256
    "B": "-fs 8000 -format_in raw -format_out raw -preset exten".split(),        # 256 / 128: two frames share a transform
    "C": SIG + PLAIN + ["-w", "25", "-s", "10", "-preem", "0.97"],               # 400 / 160: a tail entry outlives a one-frame push
    "D": SIG + PLAIN + ["-w", "32", "-s", "8", "-remove_dc", "off"],             # 512 / 128: four frames per sample
}
SHAPE = {"A": (512, 256), "B": (256, 128), "C": (400, 160), "D": (512, 128)}
ORACLE_BOUND = {"A": (2, 0.3), "B": (2, 0.3), "C": (1, 0.05), "D": (1, 0.05)}   # (max, mean) LSB: test_enhancement_output's


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


_cache = {}


def _case(Engine, name, frames=96):
    """(engine, signal, the offline run's samples) of a configuration, made once for the module and left unchanged."""
    key = (name, frames)
    if key not in _cache:
        eng = Engine(CFG[name])
        assert (eng.dims.window, eng.dims.wshift) == SHAPE[name] and eng.dims.signal_out == 1
        x = _signal(eng, frames)
        off = eng.enhance([x])[0]
        assert off.size == frames * eng.dims.wshift + eng.dims.window - eng.dims.wshift
        off.setflags(write=False)
        _cache[key] = (eng, x, off)
    return _cache[key]


def _set(eng, name, n, max_push):
    return eng.streams(n, max_push, nr_state=name in "AB", signal_state=True)


def _stream(eng, st, sid, x, chunks):
    """Pushes x in `chunks` on stream sid and finishes; the samples, after checking every push's count, st.frames and st.pending
    against ctu_streams_signal_step."""
    w, s = eng.dims.window, eng.dims.wshift
    got, at, done = [], 0, 0
    for c in chunks:
        r = st.push_signal({sid: x[at:at + c]})[sid]
        at += c
        delivered, pending = streams_signal_step(w, s, at)
        assert r.dtype == np.int16 and r.size == delivered - done, (at, c)
        assert st.frames(sid) == max(eng.num_frames(at), 0) == delivered // s and st.pending(sid) == pending, (at, c)
        done = delivered
        got.append(r.copy())
    pending = st.pending(sid)
    got.append(st.finish_signal(sid).copy())
    assert got[-1].size == pending and st.frames(sid) == 0 and st.pending(sid) == 0
    return np.concatenate(got)


def _eights(eng, x):
    """A push that completes eight frames, pushes of eight hops, the rest."""
    w, s = eng.dims.window, eng.dims.wshift
    out = [w + 7 * s]
    while sum(out) + 8 * s <= x.size:
        out.append(8 * s)
    return out + [x.size - sum(out)]


def _lsb(a, b):
    return np.abs(a.astype(int) - b.astype(int))


@pytest.mark.parametrize("name", list(CFG))
def test_pushes_of_eight_hops_are_the_offline_samples_bit_for_bit(Engine, name):
    eng, x, off = _case(Engine, name)
    w, s = eng.dims.window, eng.dims.wshift
    chunks = _eights(eng, x)
    assert chunks[:2] == [w + 7 * s, 8 * s] and len(chunks) == 13
    st = _set(eng, name, 2, w + 8 * s)
    got = _stream(eng, st, 1, x, chunks)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("name", list(CFG))
def test_any_chunking_is_within_one_lsb_of_the_offline_run_and_within_its_bound_of_the_oracle(Engine, name):
    """Share of samples that differ from the offline run, and the worst difference, measured on gfx950: DESIGN.md section 4.10 (Signal state)."""
    eng, x, off = _case(Engine, name)
    w, s = eng.dims.window, eng.dims.wshift
    st = _set(eng, name, 1, max(w, 17 * s))
    got = _stream(eng, st, 0, x, _schedule(eng, x.size, 11))
    assert got.size == 96 * s + w - s == off.size
    d = _lsb(got, off)
    ref = Oracle(CFG[name]).enhance(x)
    do = _lsb(got, ref)
    print("signal set %s: %.4f %% of the samples differ from the offline run, worst %d LSB; against the oracle max %d LSB, mean %.4f"
          % (name, 100.0 * float((d > 0).mean()), int(d.max()), int(do.max()), float(do.mean())))
    assert d.max() <= 1
    assert ref.shape == got.shape and do.max() <= ORACLE_BOUND[name][0] and do.mean() <= ORACLE_BOUND[name][1]


@pytest.mark.parametrize("name", ["A", "C"])
def test_a_streams_samples_do_not_depend_on_the_other_streams_of_its_push(Engine, name):
    eng = _case(Engine, name)[0]
    w, s = eng.dims.window, eng.dims.wshift
    n = w + 39 * s + s // 2
    xa, xb, xc, xd1, xd2 = (_signal(eng, 40 + k)[k * 37:k * 37 + n].copy() for k in range(5))
    assert len({v.tobytes() for v in (xa, xb, xc, xd1, xd2)}) == 5
    A, B, C, D = 3, 0, 2, 1
    sigs = {A: xa, B: xb, C: xc, D: xd2}
    rest = lambda x, first: first + [8 * s] * ((x.size - sum(first)) // (8 * s)) + [(x.size - sum(first)) % (8 * s)]
    plan = {A: rest(xa, [w + 7 * s]), B: rest(xb, [w + 7 * s, 8 * s]), C: rest(xc, [w + 7 * s, s // 2]), D: rest(xd2, [w + 7 * s])}
    assert all(sum(plan[k]) == sigs[k].size for k in plan)
    st = _set(eng, name, 4, w + 8 * s)
    got = {k: [] for k in plan}
    # ahead of the push in question: B and C have had a first push, D a whole file
    first = st.push_signal({B: xb[:plan[B][0]], C: xc[:plan[C][0]]})
    at = {A: 0, B: plan[B][0], C: plan[C][0], D: 0}
    step = {A: 0, B: 1, C: 1, D: 0}
    got[B].append(first[B].copy())
    got[C].append(first[C].copy())
    d1 = _stream(eng, st, D, xd1, _eights(eng, xd1))
    assert np.array_equal(d1, eng.enhance([xd1])[0])
    # the push: A starts a file, B goes on, C completes no frame, D starts its second file
    out = st.push_signal({k: sigs[k][at[k]:at[k] + plan[k][step[k]]] for k in (A, B, C, D)})
    assert [out[k].size for k in (A, B, C, D)] == [8 * s, 8 * s, 0, 8 * s]
    for k in (A, B, C, D):
        got[k].append(out[k].copy())
        at[k] += plan[k][step[k]]
        step[k] += 1
    while any(step[k] < len(plan[k]) for k in plan):
        p = {k: sigs[k][at[k]:at[k] + plan[k][step[k]]] for k in plan if step[k] < len(plan[k])}
        for k, r in st.push_signal(p).items():
            got[k].append(r.copy())
            at[k] += p[k].size
            step[k] += 1
    for k in plan:
        assert st.frames(k) == 40
        got[k].append(st.finish_signal(k).copy())
        alone = _stream(eng, _set(eng, name, 1, w + 8 * s), 0, sigs[k], plan[k])
        assert np.array_equal(np.concatenate(got[k]), alone), k
    # A and D pushed in eights from the file's start: the offline samples as well
    offl = eng.enhance([xa, xd2])
    assert np.array_equal(np.concatenate(got[A]), offl[0]) and np.array_equal(np.concatenate(got[D]), offl[1])


def test_the_second_file_of_a_stream_starts_clean(Engine):
    eng, x, off = _case(Engine, "A")
    w, s = eng.dims.window, eng.dims.wshift
    chunks = _schedule(eng, x.size, 3)
    st = _set(eng, "A", 2, max(w, 17 * s))
    first = _stream(eng, st, 1, x, chunks)
    second = _stream(eng, st, 1, x, chunks)    # the tail and the noise estimate of the first file are gone
    fresh = _stream(eng, _set(eng, "A", 2, max(w, 17 * s)), 1, x, chunks)
    assert np.array_equal(first, second) and np.array_equal(first, fresh)
    assert _lsb(first, off).max() <= 1


@pytest.mark.parametrize("name", ["C", "D"])
def test_one_frame_per_push_carries_the_tail_over_itself(Engine, name):
    """(F1 - F0) * wshift < window - wshift: a new tail entry reads an old one further on, which the same launch replaces."""
    eng, x, off = _case(Engine, name, frames=48)
    w, s = eng.dims.window, eng.dims.wshift
    chunks = [w] + [s] * 47 + [x.size - w - 47 * s]
    assert s < w - s and sum(chunks) == x.size
    got = _stream(eng, _set(eng, name, 1, w), 0, x, chunks)
    d = _lsb(got, off)
    print("one frame per push, %s: %.4f %% of the samples differ from the offline run, worst %d LSB" % (name, 100.0 * float((d > 0).mean()), int(d.max())))
    assert got.size == off.size and d.max() <= 1
    ref = Oracle(CFG[name]).enhance(x)
    do = _lsb(got, ref)
    assert do.max() <= ORACLE_BOUND[name][0] and do.mean() <= ORACLE_BOUND[name][1]
    # the same schedule as stream 1 of a two-stream set, beside a stream with other samples
    y = _signal(eng, 48, seed=9)[::-1].copy()
    st = _set(eng, name, 2, w)
    two, at = [], 0
    for c in chunks:
        two.append(st.push_signal({0: y[at:at + c], 1: x[at:at + c]})[1].copy())
        at += c
    two.append(st.finish_signal(1).copy())
    assert np.array_equal(np.concatenate(two), got)


def test_refusals_come_before_anything_changes(Engine):
    eng, x, off = _case(Engine, "A")
    w, s = eng.dims.window, eng.dims.wshift
    st = _set(eng, "A", 2, w + 8 * s)
    head = x[:w + 7 * s]
    with pytest.raises(CtuError) as ei:
        st.push_signal({0: head}, capacity=8 * s - 1)
    assert ei.value.code == ceng.CTU_ERR_INPUT and "out_capacity" in str(ei.value)
    assert st.frames(0) == 0 and st.pending(0) == 0
    got = st.push_signal({0: head}, capacity=8 * s)[0].copy()     # exactly enough
    fresh = _set(eng, "A", 2, w + 8 * s).push_signal({0: head})[0]
    assert got.size == 8 * s and np.array_equal(got, fresh) and np.array_equal(got, off[:8 * s])
    # a repeated id (the Python form keys by id: the C call)
    L = ceng.load_library()
    ids = np.array([1, 1], np.int32)
    ns = np.array([s, s], np.int64)
    ptrs = (ctypes.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
    out = np.zeros(4 * s, np.int16)
    counts = np.zeros(2, np.int64)
    rc = L.ctu_streams_push_signal_host(st._h, 2, ids.ctypes.data, ptrs, ns.ctypes.data, out.ctypes.data, out.size, counts.ctypes.data)
    assert rc == ceng.CTU_ERR_INPUT and "appears twice" in L.ctu_last_error(eng._h).decode()
    assert st.frames(1) == 0 and st.frames(0) == 8
    # the wrong call for the set
    with pytest.raises(CtuError) as ei:
        st.push({0: x[:s]})
    assert ei.value.code == ceng.CTU_ERR_INPUT and "ctu_streams_push_signal" in str(ei.value)
    with pytest.raises(CtuError) as ei:
        st.finish(0)
    assert ei.value.code == ceng.CTU_ERR_INPUT and "ctu_streams_finish_signal" in str(ei.value)
    assert st.frames(0) == 8 and st.pending(0) == w - s
    from tests.util import C2
    plain = Engine(C2)
    rows = plain.streams(2, 4000)
    with pytest.raises(CtuError) as ei:
        rows.push_signal({0: x[:2000]})
    assert ei.value.code == ceng.CTU_ERR_INPUT and "signal state" in str(ei.value)
    with pytest.raises(CtuError) as ei:
        rows.finish_signal(0)
    assert ei.value.code == ceng.CTU_ERR_INPUT
    assert rows.push({0: x[:2000]})[0].shape[0] == plain.num_frames(2000)
    # the flags a speech-output configuration behind exten needs
    with pytest.raises(CtuError) as ei:
        eng.streams(2, 4000, signal_state=True)
    assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and "-nr_mode exten" in str(ei.value)
    with pytest.raises(CtuError) as ei:
        eng.streams(2, 4000, nr_state=True)
    assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and "-format_out raw" in str(ei.value)
    # the set is as usable as before: the file goes on to the offline samples
    rest = st.push_signal({0: x[w + 7 * s:w + 15 * s]})[0]
    assert np.array_equal(rest, off[8 * s:16 * s])


def test_a_refused_row_call_between_signal_pushes_and_a_finish_changes_nothing(Engine):
    """Turn and descriptor reuse across call kinds on one set: pushes of one to three hops on a set of three streams at 256 points,
    a finish between two pushes, and a row call, which is refused and must leave the turn, the push counter and the mirrors alone."""
    eng = _case(Engine, "B")[0]
    w, s = eng.dims.window, eng.dims.wshift
    assert (w, s) == (256, 128)
    hops = {0: [3, 0, 1, 2, 0, 3], 1: [0, 2, 3, 0, 1, 2], 2: [0, 3, 0, 2, 1, 3]}   # per push (stream 1: its second file)
    first1 = _signal(eng, 4, seed=5)[:3 * s].copy()                                         # stream 1's first file: three hops, two frames
    xs = {k: _signal(eng, 16, seed=11 + k)[:sum(hops[k]) * s].copy() for k in hops}
    st = _set(eng, "B", 3, 3 * s)
    got, at = {k: [] for k in hops}, {k: 0 for k in hops}

    def push(i):
        p = {k: xs[k][at[k]:at[k] + hops[k][i] * s] for k in hops if hops[k][i]}
        for k, r in st.push_signal(p).items():
            got[k].append(r.copy())
            at[k] += p[k].size

    out = st.push_signal({0: xs[0][:3 * s], 1: first1})
    got[0].append(out[0].copy())
    at[0] = 3 * s
    file1 = np.concatenate([out[1], st.finish_signal(1)])
    assert st.frames(1) == 0 and st.pending(1) == 0
    push(1)                                                  # streams 1 and 2: stream 1 starts its second file
    before = [(st.frames(k), st.pending(k)) for k in hops]
    with pytest.raises(CtuError) as ei:
        st.push({0: xs[0][at[0]:at[0] + s]})
    assert ei.value.code == ceng.CTU_ERR_INPUT
    assert "a set with signal state (CTU_STREAMS_SIGNAL_STATE) delivers samples, not rows: use ctu_streams_push_signal / ctu_streams_finish_signal" in str(ei.value)
    assert [(st.frames(k), st.pending(k)) for k in hops] == before
    for i in range(2, 6):                                    # four more
        push(i)
    assert np.array_equal(file1, eng.enhance([first1])[0])
    off = eng.enhance([xs[k] for k in hops])
    for k in hops:
        assert at[k] == xs[k].size
        got[k].append(st.finish_signal(k).copy())
        mine = np.concatenate(got[k])
        d = _lsb(mine, off[k]) if mine.shape == off[k].shape else None
        print("stream %d: %d samples, %s differ from the offline run" % (k, mine.size, "?" if d is None else int((d > 0).sum())))
        assert mine.shape == off[k].shape and np.array_equal(mine, off[k]), k


def test_a_file_shorter_than_one_frame(Engine):
    eng, x, off = _case(Engine, "C")
    w, s = eng.dims.window, eng.dims.wshift
    st = _set(eng, "C", 2, w + 8 * s)
    assert st.push_signal({1: x[:w - s - 1]})[1].size == 0
    with pytest.raises(CtuError, match="shorter than one frame") as ei:
        st.finish_signal(1)
    assert ei.value.code == ceng.CTU_ERR_INPUT and st.frames(1) == 0 and st.pending(1) == 0
    # a file with the first samples loaded but no frame: nothing to deliver, and no error
    assert st.push_signal({1: x[:w - 1]})[1].size == 0 and st.pending(1) == 0
    assert st.finish_signal(1).size == 0
    got = _stream(eng, st, 1, x, _eights(eng, x))
    assert np.array_equal(got, off)
