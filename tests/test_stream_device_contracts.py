"""The device forms of stream sets - ctu_streams_push / _push_vad / _push_signal and the three ctu_streams_finish* without _host -
held to the buffer contracts of include/ctu_engine.h.  Every set has a twin driven through the host forms with the same chunking, and
every comparison is of bits: S1 the rows, bytes and samples of each call are the twin's, written into a guarded tensor of exactly the
capacity the counting functions name; S2 the same from d_pcm layouts the host forms never make; S3 one row or sample less room is
CTU_ERR_INPUT with nothing written and nothing changed; S4 d_pcm is only read."""
import numpy as np
import pytest

from ctucopy_amd import (CtuError, streams_config_check, streams_rows_step, streams_signal_step, streams_step, streams_vad_step)
from ctucopy_amd import engine as ceng
from tests import contracts as K
from tests.util import C2, C4, M44, SIG_EXTEN, synth_utt

pytestmark = pytest.mark.gpu

# name -> (command line, the set's flags, what a call delivers)
SETS = {
    "c2": (C2, {}, "rows"),
    "c2_da_zexp": (C2 + "-fea_delta d_a -fea_Z_exp 500".split(), dict(row_state=True), "rows"),
    "c4": (C4, dict(nr_state=True, vad_state=True), "vad"),
    "sig_exten": (SIG_EXTEN, dict(nr_state=True, signal_state=True), "signal"),
    "m44_exten": (M44 + ["-nr_mode", "exten"], dict(nr_state=True, large_state=True), "rows"),
}
N_STREAMS = 3
IDS = [2, 0, 1]   # the order of a push's streams
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    ceng.load_library()  # fails loudly when the HIP extension is missing


def _delivered(name, eng, total):
    """(rows or samples delivered, what a finish adds) of a stream of the set after `total` samples: the counting functions."""
    cfg, flags, kind = SETS[name]
    w, s = eng.dims.window, eng.dims.wshift
    if kind == "signal":
        return streams_signal_step(w, s, total)
    if kind == "vad":
        return streams_vad_step(w, s, 3, total)
    if flags.get("row_state"):
        rc, reason, halo = streams_config_check(cfg, row_state=True)
        assert rc == ceng.CTU_OK and halo == 4, (rc, reason, halo)   # -fea_delta d_a: two windows of 2
        return streams_rows_step(w, s, halo, 2, total)
    return streams_step(w, s, total)[0], 0


def case(name):
    """(engine, per-stream signals, per-stream chunk lists, the twin's outputs call by call): made once, left unchanged."""
    if name not in _cache:
        from ctucopy_amd import Engine, config_table
        cfg, flags, kind = SETS[name]
        eng = Engine(cfg)
        w, s = eng.dims.window, eng.dims.wshift
        tile = int(config_table(C2, "tile_frames")[0])
        sizes = [0, 1, s - 1, w - 1, 9 * s, (tile + 1) * s]   # the last completes more frames than a tile holds
        chunks = {k: sizes[k:] + sizes[:k] for k in range(N_STREAMS)}   # every push mixes the sizes
        xs = {k: synth_utt(40 + k, sum(sizes), fs=eng.dims.fs) for k in range(N_STREAMS)}
        assert eng.num_frames(sum(sizes)) > tile + 9
        twin = eng.streams(N_STREAMS, max(sizes), **flags)
        calls, at = [], {k: 0 for k in range(N_STREAMS)}
        for p in range(len(sizes)):
            push = {k: xs[k][at[k]:at[k] + chunks[k][p]] for k in IDS}
            if kind == "signal":
                r = twin.push_signal(push)
                calls.append((np.concatenate([r[k] for k in IDS]), None))
            elif kind == "vad":
                r = twin.push(push, want_vad=True)
                calls.append((np.concatenate([r[k][0] for k in IDS]), np.concatenate([r[k][1] for k in IDS])))
            else:
                r = twin.push(push)
                calls.append((np.concatenate([r[k] for k in IDS]), None))
            for k in IDS:
                at[k] += chunks[k][p]
        for k in IDS:
            if kind == "signal":
                calls.append((twin.finish_signal(k).copy(), None))
            elif kind == "vad":
                r, v = twin.finish(k, want_vad=True)
                calls.append((r.copy(), v.copy()))
            else:
                calls.append((twin.finish(k).copy(), None))
        twin.close()
        assert sum(c[0].shape[0] for c in calls) > 0
        _cache[name] = (eng, xs, chunks, calls, sizes)
    return _cache[name]


def tight(ns):
    """The host form's staging: one chunk behind the other."""
    off = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    return off, int(np.sum(ns)), "zeros"


def scattered(ns):
    """What the host form never makes: every chunk at an odd sample offset, in descending address order, junk between and around them."""
    off, at = np.zeros(len(ns), np.int64), 37
    for i in reversed(range(len(ns))):
        off[i] = at
        at += int(ns[i]) + 21
        at += 1 - at % 2
    assert all(o % 2 == 1 for o in off) and all(off[i] > off[i + 1] + ns[i + 1] for i in range(len(ns) - 1))
    return off, at + 64, "rails"


def drive(name, k_poison, layout, refuse=False):
    """The whole schedule through the device forms of a fresh set: each call's (rows or samples, bytes) as numpy, after checking the
    guards, the counts and d_pcm.  With `refuse`: ahead of every call that delivers something, the same call with one row or sample
    less room, which must be refused with nothing written and nothing changed."""
    import torch
    eng, xs, chunks, calls, sizes = case(name)
    cfg, flags, kind = SETS[name]
    D = eng.dims.row_floats
    st = eng.streams(N_STREAMS, max(sizes), **flags)
    dt, guard = (torch.int16, K.GUARD_SAMPLES) if kind == "signal" else (torch.float32, K.GUARD_ROWS)
    poison = K.POISON[K._dtype_name(dt)]
    got, total = [], {k: 0 for k in range(N_STREAMS)}

    def buffers(cap, k):
        whole, view = K.guarded((cap,) if kind == "signal" else (cap, D), dt, guard, poison[k])
        vw, vv = K.guarded((cap,), torch.uint8, K.GUARD_BYTES, K.POISON["uint8"][k]) if kind == "vad" else (None, None)
        return whole, view, vw, vv

    def call(fn, cap, want_counts):
        if refuse and cap > 0:
            before = [(st.frames(i), st.pending(i)) for i in range(N_STREAMS)]
            for j in range(2):
                whole, view, vw, vv = buffers(cap - 1, j)
                with pytest.raises(CtuError) as ei:
                    fn(view, vv)
                torch.cuda.synchronize()
                assert ei.value.code == ceng.CTU_ERR_INPUT
                assert (K.bits(whole) == K._word(poison[j], K.bits(whole))).all()   # entirely untouched, guards and all
                assert vw is None or (K.bits(vw) == K.POISON["uint8"][j]).all()
                assert [(st.frames(i), st.pending(i)) for i in range(N_STREAMS)] == before
        whole, view, vw, vv = buffers(cap, k_poison)
        counts = fn(view, vv)
        torch.cuda.synchronize()
        assert list(np.atleast_1d(counts)) == want_counts, (counts, want_counts)
        assert K.guards_intact(whole, view, poison[k_poison]) and (vw is None or K.guards_intact(vw, vv, K.POISON["uint8"][k_poison]))
        got.append((view.cpu().numpy(), None if vv is None else vv.cpu().numpy()))

    for p in range(len(sizes)):
        ns = np.array([chunks[k][p] for k in IDS], np.int64)
        off, size, fill = layout(ns)
        pcm_h = K.junk(size, fill)
        want = []
        for i, k in enumerate(IDS):
            pcm_h[off[i]:off[i] + ns[i]] = xs[k][total[k]:total[k] + ns[i]]
            want.append(_delivered(name, eng, total[k] + int(ns[i]))[0] - _delivered(name, eng, total[k])[0])
            total[k] += int(ns[i])
        pcm = torch.from_numpy(pcm_h).cuda()
        if kind == "signal":
            call(lambda view, vv: st.push_signal_device(IDS, pcm, off, ns, view), sum(want), want)
        else:
            call(lambda view, vv: st.push_device(IDS, pcm, off, ns, view, vad=vv), sum(want), want)
        assert K.bits_equal(pcm, pcm_h), "the push changed d_pcm"
        for k in IDS:
            assert st.pending(k) == _delivered(name, eng, total[k])[1]
    for k in IDS:
        pend = st.pending(k)
        assert pend == _delivered(name, eng, total[k])[1]
        if kind == "signal":
            call(lambda view, vv: st.finish_signal_device(k, view), pend, [pend])
        else:
            call(lambda view, vv: st.finish_device(k, view, vad=vv), pend, [pend])
        assert st.frames(k) == 0 and st.pending(k) == 0
    st.close()
    return got


def same_calls(a, b):
    return len(a) == len(b) and all(K.bits_equal(x[0], y[0]) and ((x[1] is None and y[1] is None) or K.bits_equal(x[1], y[1])) for x, y in zip(a, b))


def _shaped(eng, kind, calls):
    """The twin's outputs in the shape a device call leaves them in."""
    return [(r if kind == "signal" else r.reshape(-1, eng.dims.row_floats), v) for r, v in calls]


@pytest.mark.parametrize("name", list(SETS))
def test_s1_every_call_writes_the_twins_output_and_exactly_that(name):
    eng, xs, chunks, calls, sizes = case(name)
    a, b = drive(name, 0, tight), drive(name, 1, tight)
    twin = _shaped(eng, SETS[name][2], calls)
    assert same_calls(a, twin) and same_calls(b, twin)
    for (ra, va), (rb, vb) in zip(a, b):   # capacity words, all written
        assert K.written(ra, rb).all() and (va is None or K.written(va, vb).all())
        assert va is None or set(np.unique(va)) <= {ord("0"), ord("1")}


@pytest.mark.parametrize("name", list(SETS))
def test_s2_where_the_chunks_lie_in_d_pcm_does_not_matter(name):
    eng, xs, chunks, calls, sizes = case(name)
    assert same_calls(drive(name, 0, scattered), _shaped(eng, SETS[name][2], calls))


@pytest.mark.parametrize("name", list(SETS))
def test_s3_too_little_room_is_refused_before_anything_is_written_or_changed(name):
    eng, xs, chunks, calls, sizes = case(name)
    assert same_calls(drive(name, 1, tight, refuse=True), _shaped(eng, SETS[name][2], calls))
