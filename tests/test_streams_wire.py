"""Wire input on the GPU (include/ctu_engine.h: ctu_streams_push_wire*): G.711 codes, byte-swapped and channel-interleaved PCM pushed as
they lie in one buffer give, bit for bit, what the plain push gives for the same samples expanded on the host - rows, decisions, samples,
counts, ctu_streams_frames / ctu_streams_pending after every push, and the finish.

Every expected value comes from the existing calls (Streams.push_device / push_signal_device / push) on samples expanded here: G.711 through
the reference's own tables (tests/golden/ref_outputs.npz), the swap through numpy's byteswap.  Nothing expected goes through the code under
test.  All comparisons are of bits; there is no tolerance in this file.

1  the four formats, contiguous, on the plain chain: every residue of the carry (mod 8) against every residue of elem_off (mod 8)
2  channel-interleaved blocks, strides 5 and 64; push_interleaved
3  every kind of state a set can hold, wire and plain pushes alternating on the same streams
4  the host forms, from pageable and page-locked buffers; the limit on the covering range
5  the buffer contracts: input only read, exactly the counted output written, every refusal with its words and without effect
"""
import ctypes

import numpy as np
import pytest

from ctucopy_amd import CtuError, streams_flags_for
from ctucopy_amd import engine as ceng
from tests import contracts as K
from tests.util import C4, C5, M8, M44, SIG_EXTEN, g711_codes, ref_outputs, synth_utt

pytestmark = pytest.mark.gpu

FORMATS = ("s16", "s16_swapped", "alaw", "mulaw")
SIZES = [0, 1, 7, 8, 9, 79, 80, 81, 199, 200, 201, 1900, 2100]
ENERGY_VAD = "-vad_out_mode vad -vad_cri_mode energy -vad_thr_mode dyn".split()
SIG8 = ["-fs", "8000"] + SIG_EXTEN[2:]
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    ceng.load_library()  # fails loudly when the HIP extension is missing


# ---- inputs: what lies in the caller's buffer (raw elements) and what it is worth (samples), per format
def _table(fmt):
    return ref_outputs()["amulaw_a" if fmt == "alaw" else "amulaw_mu"]


def _raw_of(fmt, x, codes=None):
    """(raw elements, samples) of one stream: for the S16 formats from the samples x, for G.711 from `codes` (default: the codes whose
    value lies next above x in the reference's table, so that the expanded signal keeps the shape of x)."""
    if fmt == "s16":
        return x.copy(), x
    if fmt == "s16_swapped":
        return x.byteswap(), x
    t = _table(fmt)
    if codes is None:
        order = np.argsort(t, kind="stable")
        codes = order[np.clip(np.searchsorted(t[order], x), 0, 255)].astype(np.uint8)
    return codes, t[codes]


def _lay(raws, ns, at, stride, phase, chans=None, seed=0):
    """One buffer holding raws[i][at[i] : at[i] + ns[i]] for every i, and the element offsets.  stride 1: the runs one behind the other in
    descending address order with junk between them, run i starting at an element = phase + 3 i (mod 8) - odd and even offsets alike.
    stride > 1: rows of `stride` channels, run i in channel chans[i] from row i + phase on, junk in every other element."""
    dt = raws[0].dtype
    rng = np.random.default_rng(1000 + seed)
    junk = (lambda n: rng.integers(0, 256, size=n, dtype=np.uint8)) if dt == np.uint8 else (lambda n: rng.integers(-32768, 32768, size=n).astype(np.int16))
    off = np.zeros(len(raws), np.int64)
    if stride == 1:
        pos = 5
        for i in reversed(range(len(raws))):
            pos += (phase + 3 * i - pos) % 8
            off[i] = pos
            pos += int(ns[i]) + 11
        buf = junk(pos + 40)
        for i, r in enumerate(raws):
            buf[off[i]:off[i] + ns[i]] = r[at[i]:at[i] + ns[i]]
        return buf, off
    rows = int(max(ns)) + len(raws) + phase + 2
    buf = junk(rows * stride)
    for i, r in enumerate(raws):
        off[i] = (i + phase) * stride + chans[i]
        buf[off[i]:off[i] + ns[i] * stride:stride] = r[at[i]:at[i] + ns[i]]
    return buf, off


# ---- one call on a set, wire or plain, device or host form: (rows or samples, decisions or None, counts) as numpy
def _kind(flags):
    return "signal" if flags & ceng.STREAMS_SIGNAL_STATE else "vad" if flags & ceng.STREAMS_VAD_STATE else "rows"


def _capacity(st, kind, ids, ns):
    s = st.engine.dims.wshift
    if kind == "signal":
        return int(sum((int(n) // s + 1) * s for n in ns))
    return int(sum(int(n) // s + 1 + st.pending(int(k)) for k, n in zip(ids, ns)))


def _push(st, kind, ids, buf, off, ns, fmt=None, stride=1, form="device"):
    """fmt None: the plain push of int16 samples (device form).  Else a wire push of `buf`: form "device", "host" (pageable numpy) or
    "pinned" (a ctu_host_alloc buffer)."""
    import torch
    D = st.engine.dims.row_floats
    cap = _capacity(st, kind, ids, ns)
    if fmt is not None and form != "device":
        h = buf
        if form == "pinned":
            h = ceng.host_alloc(buf.shape, buf.dtype)
            h[...] = buf
        if kind == "signal":
            r = st.push_signal_wire(h, ids, off, ns, fmt=fmt, stride=stride)
            return np.concatenate([r[k] for k in ids]), None, [r[k].size for k in ids]
        r = st.push_wire(h, ids, off, ns, fmt=fmt, stride=stride, want_vad=kind == "vad")
        assert np.array_equal(h, buf), "the push changed h_in"
        if kind == "vad":
            return np.concatenate([r[k][0] for k in ids]), np.concatenate([r[k][1] for k in ids]), [r[k][0].shape[0] for k in ids]
        return np.concatenate([r[k] for k in ids]), None, [r[k].shape[0] for k in ids]
    dev = torch.from_numpy(buf).cuda()
    if kind == "signal":
        out = torch.zeros(max(cap, 1), dtype=torch.int16, device="cuda")
        counts = (st.push_signal_device(ids, dev, off, ns, out) if fmt is None
                  else st.push_signal_wire_device(ids, dev, off, ns, out, fmt=fmt, stride=stride))
        torch.cuda.synchronize()
        assert K.bits_equal(dev, buf), "the push changed d_in"
        return out[:int(counts.sum())].cpu().numpy(), None, [int(c) for c in counts]
    rows = torch.zeros((max(cap, 1), D), dtype=torch.float32, device="cuda")
    vad = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda") if kind == "vad" else None
    counts = (st.push_device(ids, dev, off, ns, rows, vad=vad) if fmt is None
              else st.push_wire_device(ids, dev, off, ns, rows, fmt=fmt, stride=stride, vad=vad))
    torch.cuda.synchronize()
    assert K.bits_equal(dev, buf), "the push changed d_in"
    n = int(counts.sum())
    return rows[:n].cpu().numpy(), None if vad is None else vad[:n].cpu().numpy(), [int(c) for c in counts]


def _finish(st, kind, k):
    if kind == "signal":
        return st.finish_signal(k).copy(), None
    if kind == "vad":
        r, v = st.finish(k, want_vad=True)
        return r.copy(), v.copy()
    return st.finish(k).copy(), None


def _run(st, kind, ids, raws, xs, schedule, wire):
    """A file per stream through `schedule` (a list of per-stream counts, in the order of ids) and the finishes: everything every call
    delivered, and (frames, pending) of every stream behind it.  wire(p) says how push p goes: None (plain: the samples xs, contiguous)
    or (fmt, stride, phase, chans, form)."""
    got, at = [], [0] * len(ids)
    for p, ns in enumerate(schedule):
        ns = np.asarray(ns, np.int64)
        how = wire(p)
        if how is None:
            buf, off = _lay(xs, ns, at, 1, p % 8, seed=p)
            out = _push(st, kind, ids, buf, off, ns)
        else:
            fmt, stride, phase, chans, form = how
            buf, off = _lay(raws, ns, at, stride, phase, chans, seed=p)
            out = _push(st, kind, ids, buf, off, ns, fmt=fmt, stride=stride, form=form)
        at = [a + int(n) for a, n in zip(at, ns)]
        got.append(out + ([(st.frames(k), st.pending(k)) for k in ids],))
    for k in ids:
        got.append(_finish(st, kind, k) + ([], [(st.frames(j), st.pending(j)) for j in ids]))
    return got


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert K.bits_equal(x[0], y[0]), ("rows or samples of call", i)
        assert (x[1] is None and y[1] is None) or K.bits_equal(x[1], y[1]), ("decisions of call", i)
        assert x[2:] == y[2:], ("counts, frames or pending behind call", i, x[2:], y[2:])


# ---- case 1: the plain chain at 8 kHz, three streams, the thirteen sizes in a fixed shuffled order per stream
IDS1 = [2, 0, 1]


def _inputs1(fmt):
    """(raw elements, samples, schedule) of a format: no engine, no device."""
    rng = np.random.default_rng(8)
    orders = [rng.permutation(len(SIZES)) for _ in IDS1]
    schedule = [[SIZES[orders[i][p]] for i in range(len(IDS1))] for p in range(len(SIZES))]
    total = sum(SIZES)
    if fmt.startswith("s16"):
        xs = [synth_utt(70 + i, total, fs=8000) for i in range(len(IDS1))]
        return [_raw_of(fmt, x)[0] for x in xs], xs, schedule
    codes = [g711_codes(total + i)[i:] for i in range(len(IDS1))]
    codes[0] = np.concatenate([np.arange(256, dtype=np.uint8), codes[0][256:]])
    return codes, [_raw_of(fmt, None, c)[1] for c in codes], schedule


def _case1(fmt):
    """(engine, raw elements, samples, schedule, the plain run's calls) of a format: made once, left unchanged."""
    key = "pcm" if fmt.startswith("s16") else fmt
    if ("c1", key) not in _cache:
        from ctucopy_amd import Engine
        if "m8" not in _cache:
            _cache["m8"] = Engine(M8)
        eng = _cache["m8"]
        assert (eng.dims.window, eng.dims.wshift, eng.dims.wfft) == (200, 80, 256)
        codes, xs, schedule = _inputs1(fmt)
        st = eng.streams(3, max(SIZES))
        calls = _run(st, "rows", IDS1, None, xs, schedule, lambda p: None)
        st.close()
        assert 40 <= sum(c[0].shape[0] for c in calls) // 3 <= 70
        _cache[("c1", key)] = (eng, xs, schedule, calls)
    eng, xs, schedule, calls = _cache[("c1", key)]
    return eng, _inputs1(fmt)[0], xs, schedule, calls


def test_the_schedule_of_case_1_meets_what_it_is_there_for():
    """Host arithmetic only: over the eight phases every residue of the carry meets every residue of elem_off; slots cross the 2048-sample
    slice of a stitch workgroup; a push with samples completes no frame and one completes 26."""
    from ctucopy_amd import streams_step
    raws, xs, schedule = _inputs1("alaw")
    frames = lambda t: streams_step(200, 80, t)[0]
    met, frames_of, longest = set(), set(), 0
    for phase in range(8):
        at = [0] * 3
        for p, ns in enumerate(schedule):
            buf, off = _lay(raws, ns, at, 1, phase, seed=p)
            for i in range(3):
                F = frames(at[i])
                carry = at[i] - F * 80
                if ns[i]:
                    met.add((carry % 8, int(off[i]) % 8))
                    frames_of.add(frames(at[i] + ns[i]) - F)
                    longest = max(longest, 8 + carry + ns[i])
                    assert np.array_equal(buf[off[i]:off[i] + ns[i]], raws[i][at[i]:at[i] + ns[i]])
            at = [a + n for a, n in zip(at, ns)]
    assert len(met) == 64, sorted(met)
    assert 0 in frames_of and 26 in frames_of and longest > 2048
    assert np.array_equal(raws[0][:256], np.arange(256))


@pytest.mark.parametrize("fmt", FORMATS)
def test_1_contiguous_sources_give_the_rows_of_the_plain_push(fmt):
    eng, raws, xs, schedule, calls = _case1(fmt)
    st = eng.streams(3, max(SIZES))
    for phase in range(8):   # a file per phase on the same set: the finishes between them reset the streams
        _same(_run(st, "rows", IDS1, raws, xs, schedule, lambda p: (fmt, 1, phase, None, "device")), calls)
    assert st.last_push_ms()[0] >= 0.0
    st.close()


# ---- case 2: three of the channels of an interleaved block, ids in descending order, a different count per stream
IDS2, CHANS2 = [2, 1, 0], [4, 0, 2]
BLOCKS2 = [7, 650, 81, 2100, 1200, 400]


def _case2(fmt):
    key = "pcm" if fmt.startswith("s16") else fmt
    if ("c2", key) not in _cache:
        eng = _case1(fmt)[0]
        schedule = [[max(b - d, 0) for d in (0, 3, 9)] for b in BLOCKS2]
        total = sum(BLOCKS2)
        pcm = [synth_utt(90 + i, total, fs=8000) for i in range(3)]
        pairs = [_raw_of("s16" if key == "pcm" else fmt, x) for x in pcm]
        xs = [p[1] for p in pairs]
        st = eng.streams(3, max(BLOCKS2))
        calls = _run(st, "rows", IDS2, None, xs, schedule, lambda p: None)
        st.close()
        assert 40 <= sum(c[0].shape[0] for c in calls) // 3 <= 70
        _cache[("c2", key)] = (eng, [p[0] for p in pairs], xs, schedule, calls)
    eng, raws, xs, schedule, calls = _cache[("c2", key)]
    return eng, ([x.byteswap() for x in xs] if fmt == "s16_swapped" else raws), xs, schedule, calls


@pytest.mark.parametrize("stride", [5, 64])
@pytest.mark.parametrize("fmt", FORMATS)
def test_2_interleaved_sources_give_the_rows_of_the_plain_push(fmt, stride):
    eng, raws, xs, schedule, calls = _case2(fmt)
    st = eng.streams(3, max(BLOCKS2))
    _same(_run(st, "rows", IDS2, raws, xs, schedule, lambda p: (fmt, stride, p % 3, CHANS2, "device")), calls)
    st.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_2_push_interleaved_is_push_of_the_columns(fmt):
    eng, raws, xs, schedule, calls = _case2(fmt)
    a, b = eng.streams(5, 700), eng.streams(5, 700)
    ids = [3, 0, 4]
    at = 0
    for n in (7, 650, 81, 700, 333):
        block = np.stack([r[at:at + n] for r in raws], axis=1).copy()   # [samples, 3 channels]
        got = a.push_interleaved(block, ids=ids, fmt=fmt)
        want = b.push({k: x[at:at + n] for k, x in zip(ids, xs)})
        for k in ids:
            assert K.bits_equal(got[k], want[k]) and a.frames(k) == b.frames(k) and a.pending(k) == b.pending(k)
        at += n
    assert a.frames(3) > 15
    whole = np.stack([r[:500] for r in raws] + [raws[0][:500], raws[1][:500]], axis=1).copy()   # the default ids: channel j to stream j
    a.close(), b.close()
    a, b = eng.streams(5, 700), eng.streams(5, 700)
    got, want = a.push_interleaved(whole, fmt=fmt), b.push({j: (xs + xs[:2])[j][:500] for j in range(5)})
    assert all(K.bits_equal(got[j], want[j]) and got[j].shape[0] == 4 for j in range(5))
    a.close(), b.close()


# ---- case 3: every kind of state once; wire and plain pushes alternate on the same streams
# name -> (command line, format, stride, streams, frames per stream)
STATES = {
    "row": (M8 + "-fea_delta d_a -fea_Z_exp 500".split(), "alaw", 1, 3, 50),
    "noise + detector": (C4, "mulaw", 2, 2, 50),
    "detector behind row": (M8 + ENERGY_VAD + ["-vad_filter_order", "3", "-fea_delta", "d_a"], "alaw", 1, 3, 50),
    "signal": (SIG8, "mulaw", 1, 3, 50),
    "subtraction": (M8 + "-nr_mode fwss -vad burg".split(), "alaw", 1, 3, 50),
    "trap": (C5, "s16_swapped", 1, 2, 51),   # 51 frames: C5's shortest legal file
    "large + noise": (M44 + ["-nr_mode", "exten"], "s16_swapped", 2, 2, 12),
}


@pytest.mark.parametrize("name", list(STATES))
def test_3_wire_and_plain_pushes_alternate_on_every_kind_of_state(name):
    from ctucopy_amd import Engine
    cfg, fmt, stride, n, frames = STATES[name]
    rc, flags, reason, halo = streams_flags_for(cfg)
    assert rc == ceng.CTU_OK, reason
    kind = _kind(flags)
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    total = w + (frames - 1) * s + (0 if name == "trap" else s // 3)
    # cut so that not every push ends a multiple of eight frames into the file: 3, 11, 12, 29 ... frames, and pushes that complete none
    cuts = sorted({min(c, total) for c in (5, w + 2 * s, w + 2 * s + 1, w + 10 * s + 7, w + 11 * s, w + 28 * s + s // 2, total)})
    sizes = [b - a for a, b in zip([0] + cuts[:-1], cuts)]
    schedule = [[sizes[(p + i) % len(sizes)] for i in range(n)] for p in range(len(sizes))]   # every stream gets every size: `total` each
    ids = list(reversed(range(n)))
    pairs = [_raw_of(fmt, synth_utt(30 + i, total, fs=eng.dims.fs)) for i in range(n)]
    raws, xs = [p[0] for p in pairs], [p[1] for p in pairs]
    chans = list(range(n))
    a = eng.streams_ex(n, max(sizes), flags)
    plain = _run(a, kind, ids, raws, xs, schedule, lambda p: None)
    a.close()
    assert sum(c[0].shape[0] for c in plain) > 0
    assert kind != "vad" or all(set(np.unique(c[1])) <= {ord("0"), ord("1")} for c in plain)
    b = eng.streams_ex(n, max(sizes), flags)
    mixed = _run(b, kind, ids, raws, xs, schedule, lambda p: (fmt, stride, p % 8, chans, "device") if p % 2 == 0 else None)
    b.close()
    _same(mixed, plain)
    eng.close()


# ---- case 4: the host forms
@pytest.mark.parametrize("form", ["host", "pinned"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_4_the_host_form_delivers_the_device_forms_bits(fmt, form):
    eng, raws, xs, schedule, calls = _case1(fmt)
    st = eng.streams(3, max(SIZES))
    _same(_run(st, "rows", IDS1, raws, xs, schedule, lambda p: (fmt, 1, (3 * p + 1) % 8, None, form)), calls)
    st.close()
    eng, raws, xs, schedule, calls = _case2(fmt)
    st = eng.streams(6, max(BLOCKS2))   # (a block of five channels is up to 5 * max_push elements and a row: a set of six streams stages it)
    _same(_run(st, "rows", IDS2, raws, xs, schedule, lambda p: (fmt, 5, p % 3, CHANS2, form)), calls)
    st.close()


@pytest.mark.parametrize("fmt", ["s16", "alaw"])
def test_4_the_covering_range_of_a_host_push_is_what_the_set_can_stage(fmt):
    eng, raws, xs, schedule, calls = _case1(fmt)
    n_streams, max_push = 3, 300
    cap = n_streams * max_push
    st, twin = eng.streams(n_streams, max_push), eng.streams(n_streams, max_push)
    buf = np.concatenate([raws[0][:cap], raws[1][:8]])
    ids, ns = [1, 2], [250, 2]
    want = twin.push({1: xs[0][:250], 2: xs[0][cap - 2:cap]})
    with pytest.raises(CtuError) as ei:   # elements 0 .. cap: one more than the set stages
        st.push_wire(buf, ids, [0, cap - 1], ns, fmt=fmt)
    assert ei.value.code == ceng.CTU_ERR_INPUT and "covering range" in str(ei.value) and "n_streams * max_push_samples" in str(ei.value)
    assert [st.frames(k) for k in ids] == [0, 0] and ceng.wire_extent([0, cap - 1], ns, fmt) == (cap + 1, 0)
    got = st.push_wire(buf, ids, [0, cap - 2], ns, fmt=fmt)   # elements 0 .. cap - 1
    assert ceng.wire_extent([0, cap - 2], ns, fmt) == (cap, 0)
    assert all(K.bits_equal(got[k], want[k]) for k in ids) and got[1].shape[0] == 1
    # ... wherever in the buffer the range starts
    got = st.push_wire(np.concatenate([buf[:7], buf]), [0], [7 + cap - 100], [100], fmt=fmt)
    want = twin.push({0: xs[0][cap - 100:cap]})
    assert K.bits_equal(got[0], want[0])
    st.close(), twin.close()


# ---- case 5: the buffer contracts of the device forms, on a set with rows and decisions and on one with samples
SETS5 = {"c4": (C4, "mulaw", 2), "sig": (SIG8, "s16_swapped", 1)}
REFUSALS = [   # (what is wrong, a word of the refusal)
    ("null layout", "null layout"), ("format 4", "unknown format"), ("format -1", "unknown format"), ("stride 0", "stride below 1"),
    ("negative offset", "negative"), ("odd address", "2-byte aligned"), ("repeat", "appears twice"), ("foreign id", "out of range"),
    ("too many samples", "max_push_samples"), ("no room", "do not fit"), ("wrong family", "signal state"),
]


def _raw_call(st, kind, ids, ptr, off, ns, layout, out, vad, family=None):
    """The C call itself, for what the binding would not pass on: a NULL layout, a buffer at an odd address."""
    import torch
    L = ceng.load_library()
    ids, off, ns = np.asarray(ids, np.int32), np.asarray(off, np.int64), np.asarray(ns, np.int64)
    counts = np.zeros(max(ids.size, 1), np.int64)
    s = torch.cuda.current_stream().cuda_stream
    w = None if layout is None else ctypes.byref(ceng.WireLayout(*layout))
    if (family or kind) == "signal":
        cap = out.numel()
        rc = L.ctu_streams_push_signal_wire(st._h, int(ids.size), ids.ctypes.data, ptr, off.ctypes.data, ns.ctypes.data, w, out.data_ptr(), cap,
                                            counts.ctypes.data, s)
    else:
        cap = out.numel() // max(st.engine.dims.row_floats, 1) if out.dtype == torch.float32 else out.numel()   # (a signal engine has no rows)
        rc = L.ctu_streams_push_wire(st._h, int(ids.size), ids.ctypes.data, ptr, off.ctypes.data, ns.ctypes.data, w, out.data_ptr(), cap,
                                     counts.ctypes.data, None if vad is None else vad.data_ptr(), s)
    return rc, L.ctu_last_error(st.engine._h).decode(), counts[:ids.size]


def _drive5(name, k_poison, refusing):
    import torch
    from ctucopy_amd import Engine
    cfg, fmt, stride = SETS5[name]
    if ("e5", name) not in _cache:
        _cache[("e5", name)] = Engine(cfg)
    eng = _cache[("e5", name)]
    rc, flags, reason, halo = streams_flags_for(cfg)
    assert rc == ceng.CTU_OK, reason
    kind = _kind(flags)
    code = ceng.WIRE_FORMATS[fmt]
    w, s, D = eng.dims.window, eng.dims.wshift, eng.dims.row_floats
    sizes = [5, w + 2 * s, 1, 9 * s + 7, 24 * s, 0, 3 * s - 1]
    ids = [1, 0]
    pairs = [_raw_of(fmt, synth_utt(50 + i, sum(sizes), fs=eng.dims.fs)) for i in range(2)]
    raws = [p[0] for p in pairs]
    st = eng.streams_ex(2, max(sizes), flags)
    dt, guard = (torch.int16, K.GUARD_SAMPLES) if kind == "signal" else (torch.float32, K.GUARD_ROWS)
    poison = K.POISON[K._dtype_name(dt)][k_poison]
    vpoison = K.POISON["uint8"][k_poison]
    got, at = [], [0, 0]
    for p, n0 in enumerate(sizes):
        ns = np.array([n0, sizes[(p + 3) % len(sizes)] if p < 4 else 0], np.int64)
        buf, off = _lay(raws, ns, at, stride, p % 8, chans=[0, 1], seed=p)
        dev = torch.from_numpy(buf).cuda()
        before = [(st.frames(k), st.pending(k)) for k in ids]
        cap = _capacity(st, kind, ids, ns)
        if refusing:
            for what, word in REFUSALS:
                whole, view = K.guarded((cap,) if kind == "signal" else (cap, D), dt, guard, poison)
                vw, vv = K.guarded((cap,), torch.uint8, K.GUARD_BYTES, vpoison) if kind == "vad" else (None, None)
                a = dict(ids=ids, ptr=dev.data_ptr(), off=off, ns=ns, layout=(code, stride), out=view, vad=vv)
                if what == "null layout":
                    a["layout"] = None
                elif what.startswith("format"):
                    a["layout"] = (int(what.split()[1]), stride)
                elif what == "stride 0":
                    a["layout"] = (code, 0)
                elif what == "negative offset":
                    if ns[0] == 0:
                        continue
                    a["off"] = np.array([-1, off[1]])
                elif what == "odd address":
                    if fmt in ("alaw", "mulaw"):
                        continue   # codes lie at any address
                    a["ptr"] = dev.data_ptr() + 1
                elif what == "repeat":
                    a["ids"] = [1, 1]
                elif what == "foreign id":
                    a["ids"] = [1, 2]
                elif what == "too many samples":
                    a["ns"] = np.array([max(sizes) + 1, 0])
                elif what == "no room":
                    if _delivers(eng, kind, at, ns) == 0:
                        continue
                    short = _delivers(eng, kind, at, ns) - 1
                    a["out"] = view.reshape(-1)[:short * (1 if kind == "signal" else D)]
                elif what == "wrong family":
                    a["family"] = "rows" if kind == "signal" else "signal"
                    if kind != "signal":
                        a["out"] = torch.zeros(64, dtype=torch.int16, device="cuda")
                        a["vad"] = None
                    else:
                        a["out"] = torch.zeros(64, dtype=torch.float32, device="cuda")
                rc, words, _ = _raw_call(st, kind, **a)
                torch.cuda.synchronize()
                assert rc == ceng.CTU_ERR_INPUT, (what, rc)
                assert word in words, (what, words)
                assert (K.bits(whole) == K._word(poison, K.bits(whole))).all() and (vw is None or (K.bits(vw) == vpoison).all()), what
                assert [(st.frames(k), st.pending(k)) for k in ids] == before, what
        whole, view = K.guarded((cap,) if kind == "signal" else (cap, D), dt, guard, poison)
        vw, vv = K.guarded((cap,), torch.uint8, K.GUARD_BYTES, vpoison) if kind == "vad" else (None, None)
        rc, words, counts = _raw_call(st, kind, ids, dev.data_ptr(), off, ns, (code, stride), view, vv)
        torch.cuda.synchronize()
        assert rc == ceng.CTU_OK, words
        assert int(counts.sum()) == _delivers(eng, kind, at, ns) <= cap
        assert K.bits_equal(dev, buf), "the push changed d_in"
        assert K.guards_intact(whole, view, poison) and (vw is None or K.guards_intact(vw, vv, vpoison))
        got.append((view.cpu().numpy(), None if vv is None else vv.cpu().numpy(), [int(c) for c in counts]))
        at = [a + int(n) for a, n in zip(at, ns)]
    for k in ids:
        got.append(_finish(st, kind, k) + ([],))
    st.close()
    return got


def _delivers(eng, kind, at, ns):
    """Rows (samples) a push of ns new samples delivers behind `at` samples per stream: the counting functions of include/ctu_engine.h
    (C4: the majority filter of order 3 holds one frame back; the signal set delivers wshift samples per frame)."""
    from ctucopy_amd import streams_signal_step, streams_vad_step
    w, s = eng.dims.window, eng.dims.wshift
    step = (lambda t: streams_signal_step(w, s, t)[0]) if kind == "signal" else (lambda t: streams_vad_step(w, s, 3, t)[0])
    return sum(step(a + int(n)) - step(a) for a, n in zip(at, ns))


@pytest.mark.parametrize("name", list(SETS5))
def test_5_exactly_the_counted_output_is_written_and_a_refusal_changes_nothing(name):
    a, b = _drive5(name, 0, False), _drive5(name, 1, True)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        n = sum(x[2]) if x[2] else x[0].shape[0]
        assert x[2] == y[2]
        ra, rb = x[0].reshape(x[0].shape[0], max(x[0].size // max(x[0].shape[0], 1), 1)), y[0].reshape(y[0].shape[0], max(y[0].size // max(y[0].shape[0], 1), 1))
        assert K.bits_equal(ra[:n], rb[:n]), "a refusal changed what a later call delivers"
        if x[2]:   # a push into a guarded view of capacity rows: the counted ones written, the rest of the view left alone
            assert K.written(ra[:n], rb[:n]).all() and K.untouched(ra[n:], rb[n:], *K.POISON[str(ra.dtype)]).all()
            if x[1] is not None:
                assert K.bits_equal(x[1][:n], y[1][:n]) and K.untouched(x[1][n:], y[1][n:], *K.POISON["uint8"]).all()
                assert set(np.unique(x[1][:n])) <= {ord("0"), ord("1")}
    assert sum(sum(x[2]) for x in a if x[2]) > 0


def test_5_a_vad_buffer_is_refused_on_a_set_without_detector_state():
    import torch
    eng, raws, xs, schedule, calls = _case1("alaw")
    st, twin = eng.streams(3, 400), eng.streams(3, 400)
    dev = torch.from_numpy(raws[0][:400].copy()).cuda()
    rows, vad = torch.zeros((8, eng.dims.row_floats), device="cuda"), torch.full((8,), 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(CtuError) as ei:
        st.push_wire_device([1], dev, [1], [399], rows, fmt="alaw", vad=vad)
    torch.cuda.synchronize()
    assert ei.value.code == ceng.CTU_ERR_INPUT and "without detector state" in str(ei.value)
    assert st.frames(1) == 0 and not rows.any() and (vad == 7).all()
    counts = st.push_wire_device([1], dev, [1], [399], rows, fmt="alaw")
    want = twin.push({1: xs[0][1:400]})[1]
    torch.cuda.synchronize()
    assert counts.tolist() == [3] and K.bits_equal(rows[:3].cpu().numpy(), want)
    assert K.bits_equal(st.finish(1), twin.finish(1))
    st.close(), twin.close()
