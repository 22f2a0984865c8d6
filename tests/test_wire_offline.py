"""Offline wire input on the GPU (include/ctu_engine.h: ctu_plan_unpack_wire, ctu_engine_run_wire_host, ctu_engine_run_signal_wire_host):
a plan's utterances read out of G.711 codes, byte-swapped and strided PCM as they lie in one buffer give, bit for bit, what the plain
calls give for the same samples expanded on the host - rows, VAD bytes, speech samples, rows_per_utt.

Every expected value is Engine.extract / Engine.enhance on the samples of wire_expand (pinned by tests/test_streams_wire_cpu.py); nothing
expected goes through the code under test.  All comparisons are of bits; there is no tolerance in this file.

Shapes: the smallest at which the unpack can go wrong.  A batch is five utterances of at most half a second: window - 1 samples (no
frame), window, window + k hop + r with r through 0, 1, 7, 15, 17, and one that names the very elements of another (overlap).  They lie
in descending address order with junk between them, the first element of each at 0, 1, 3, 15, 16, 17 elements past a 16-byte boundary,
and the last element named is the last of the buffer (of the numpy array and of the tensor; the allocation behind a tensor is
rounded up).  The four formats and strides 1, 2, 3 are dealt over the engines: every pair occurs once.  An utterance of 0 samples, whose elem_off is -1, has a test of its own on an engine whose hop is its window:
ctu_plan_create takes no file shorter than window - hop samples ("IO: Signal shorter than one frame!"), so on every other engine here
such a plan does not exist.
"""
import ctypes

import numpy as np
import pytest

from ctucopy_amd import CtuError
from ctucopy_amd import engine as ceng
from tests import contracts as K
from tests.test_rows_in_cpu import HTK
from tests.util import C2, C4, M8, M44, REF_E2E_CASES, SIG_EXTEN, synth_utt

pytestmark = pytest.mark.gpu

FWSS = REF_E2E_CASES["c2_fwss"][0]
HOP = C2 + ["-w", "10", "-s", "10"]   # window = hop: a file of 0 samples is a file without a frame
# name -> (command line, sampling rate, frames of the longest utterance, [(format, stride)])
ENGINES = {
    "c2": (C2, 16000, 40, [("s16", 1), ("alaw", 2), ("s16_swapped", 3), ("mulaw", 1)]),       # 512 points
    "m8": (M8, 8000, 30, [("alaw", 1), ("s16", 2)]),                                           # the 8 kHz 256-point preset
    "w40": (REF_E2E_CASES["c2_w40"][0], 16000, 9, [("s16_swapped", 1), ("mulaw", 3)]),         # 1024 points, wave1k_kernel
    "m44": (M44, 44100, 3, [("mulaw", 2), ("s16", 3)]),                                        # bigfft_kernel<8>, three frames
    "c4": (C4, 8000, 45, [("alaw", 3), ("s16_swapped", 2)]),                                   # exten + the fused VAD: bytes too
    "sig": (SIG_EXTEN, 16000, 30, [("s16_swapped", 1), ("mulaw", 2)]),                         # speech output
}
COMBOS = [(name, fmt, stride) for name, e in ENGINES.items() for fmt, stride in e[3]]
MODS = (0, 1, 3, 15, 16, 17)   # elements past a 16-byte boundary
_engines = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    ceng.load_library()  # fails loudly when the HIP extension is missing
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def _engine(name):
    if name not in _engines:
        cfg = FWSS if name == "fwss" else HOP if name == "hop" else ENGINES[name][0]
        _engines[name] = ceng.Engine(cfg)
    return _engines[name]


OVERLAP = (4, 1)   # utterance 4 names the elements of utterance 1


def _lengths(dims, most):
    """[window - 1, long + 1, window, shorter + 7, the second again, ... + 15, + 17, + 0]: see the module's text."""
    w, h = dims.window, dims.wshift
    a = w + (most - 1) * h + 1
    return [w - 1, a, w, w + max(most // 2 - 1, 0) * h + 7, a, w + h + 15, w + 2 * h + 17, w + 3 * h]


def _junk(dtype, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, n, dtype=np.uint8) if dtype == np.uint8 else rng.integers(-32768, 32768, n).astype(np.int16)


def _lay(ns, fmt, stride, fs, seed=0, pick=None):
    """(buffer, elem_off, samples): utterance i is ns[i] elements, `stride` apart, of a buffer of junk; descending, utterance 4 at the
    elements of utterance 1, an utterance without samples at -1, first elements at MODS past a 16-byte boundary, the last element named
    the last of the buffer.  The named elements are drawn from `pick` (default: the seed of the junk), so two junk fillings can share them."""
    dt = np.uint8 if fmt in ("alaw", "mulaw") else np.int16
    per16 = 16 // np.dtype(dt).itemsize
    off = np.zeros(len(ns), np.int64)
    pos, k = 3, 0
    twin = OVERLAP[0] if len(ns) > OVERLAP[0] and ns[OVERLAP[0]] == ns[OVERLAP[1]] else -1
    for i in reversed(range(len(ns))):
        if ns[i] == 0:
            off[i] = -1
            continue
        if i == twin:
            continue
        m = MODS[k % len(MODS)]
        k += 1
        pos += (m - pos) % per16 if m < per16 else (m - pos) % per16 + per16
        assert pos % per16 == m % per16
        off[i] = pos
        pos += (int(ns[i]) - 1) * stride + 1 + 5
    if twin >= 0:
        off[twin] = off[OVERLAP[1]]
    total = max(int(off[i]) + (int(ns[i]) - 1) * stride + 1 for i in range(len(ns)) if ns[i])
    buf = _junk(dt, total, 77 + seed)
    named = np.zeros(total, bool)
    for i, n in enumerate(ns):
        if n:
            named[off[i]:off[i] + (int(n) - 1) * stride + 1:stride] = True
    if fmt in ("alaw", "mulaw"):
        vals = _junk(dt, total, 5 if pick is None else pick)
    else:  # speech-like, so that the detectors and the subtraction have something to decide on
        vals = synth_utt(5 if pick is None else pick, total, fs=fs)
        if fmt == "s16_swapped":
            vals = vals.byteswap()
    buf[named] = vals[named]
    assert named[-1]
    samples = [ceng.wire_expand(buf, max(int(o), 0), int(n), fmt=fmt, stride=stride) for o, n in zip(off, ns)]
    return np.ascontiguousarray(buf), off, samples


def _g711_speech(fmt, x):
    """Codes whose expansion follows x (G.711 inputs that are speech, for the engines whose state depends on it)."""
    t = np.array([int(ceng.wire_expand(np.array([c], np.uint8), 0, 1, fmt=fmt)[0]) for c in range(256)])
    order = np.argsort(t, kind="stable")
    return order[np.clip(np.searchsorted(t[order], x), 0, 255)].astype(np.uint8)


def _same(a, b):
    return len(a) == len(b) and all(K.bits_equal(x, y) for x, y in zip(a, b))


def _unpack(eng, plan, buf, off, fmt, stride, samples, shift=0):
    """The device form into a guarded, poisoned arena `shift` samples past a 64-byte boundary; checks what it wrote.  Returns the arena."""
    import torch
    dev = torch.from_numpy(buf).cuda()
    p = K.POISON["int16"][0]
    whole, view = K.guarded(plan.total_samples + 32, torch.int16, K.GUARD_SAMPLES, p)
    pcm = view[shift:shift + plan.total_samples]
    got = eng.unpack_wire_device(plan, dev, off, fmt=fmt, stride=stride, pcm=pcm)
    torch.cuda.synchronize()
    assert got.data_ptr() == pcm.data_ptr()
    assert K.bits_equal(dev, buf), "the unpack changed d_in"
    assert K.guards_intact(whole, view, p)
    want = np.full(plan.total_samples + 32, p, np.int16)
    for s, o in zip(samples, plan.sample_off[:-1]):
        want[shift + o:shift + o + len(s)] = s
    assert np.array_equal(view.cpu().numpy(), want), "d_pcm: the samples at the plan's offsets, the poison everywhere else"
    return pcm


def _run_device(eng, plan, pcm):
    """The plain device run of an arena: (rows or speech, VAD bytes or None) as numpy."""
    import torch
    if eng.dims.signal_out:
        out = eng.enhance_device(plan, pcm)
        torch.cuda.synchronize()
        return out.cpu().numpy(), None
    vad = torch.zeros(max(plan.total_frames, 1), dtype=torch.uint8, device="cuda") if eng.dims.has_vad else None
    rows = eng.run_device(plan, pcm, rows=torch.zeros((plan.total_frames, eng.dims.row_floats), dtype=torch.float32, device="cuda"), vad=vad)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), (vad.cpu().numpy()[:plan.total_frames] if vad is not None else None)


def _run_host(eng, plan, samples, buf=None, off=None, fmt=None, stride=1):
    """The host form of a plan, plain (buf None: the packed arena of `samples`) or wire: (rows or speech, VAD bytes or None, rows per
    utterance or None) as numpy."""
    L = ceng.load_library()
    if eng.dims.signal_out:
        out = np.zeros(plan.total_samples, dtype=np.int16)
        if buf is None:
            eng._check(L.ctu_engine_run_signal_host(eng._h, plan._h, plan.pack(samples).ctypes.data, out.ctypes.data))
        else:
            o, w = np.ascontiguousarray(off, dtype=np.int64), ceng.WireLayout(ceng.WIRE_FORMATS[fmt], stride)
            eng._check(L.ctu_engine_run_signal_wire_host(eng._h, plan._h, buf.ctypes.data, o.ctypes.data, ctypes.byref(w), out.ctypes.data))
        return out, None, None
    if buf is None:
        return eng.run_host(plan, plan.pack(samples), want_vad=True)
    return eng.run_wire_host(plan, buf, off, fmt=fmt, stride=stride, want_vad=True)


def _equal(a, b):
    return all((x is None and y is None) or K.bits_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("name,fmt,stride", COMBOS, ids=[f"{n}-{f}-{s}" for n, f, s in COMBOS])
def test_wire_equals_plain(name, fmt, stride):
    """Host form = plain call on the expanded samples; device form = host form; the buffers' contracts; junk changes no bit."""
    import torch
    eng = _engine(name)
    _, fs, most, _ = ENGINES[name]
    ns = _lengths(eng.dims, most)[:5]
    buf, off, samples = _lay(ns, fmt, stride, fs)
    assert off[4] == off[1] and off[0] > off[1] > off[2] > off[3] > 0
    keep = buf.copy()
    plan = eng.plan(ns)
    assert plan.total_frames > 0
    want = _run_host(eng, plan, samples)
    got = _run_host(eng, plan, samples, buf, off, fmt, stride)
    assert np.array_equal(buf, keep), "the run changed h_in"
    assert _equal(got, want)
    # page-locked input
    pin = ceng.host_alloc(buf.shape, buf.dtype)
    pin[...] = buf
    assert _equal(_run_host(eng, plan, samples, pin, off, fmt, stride), want)
    # the device form: what it writes; the run behind it is the plain device run of the packed arena, and the host form's
    dev = _run_device(eng, plan, _unpack(eng, plan, buf, off, fmt, stride, samples))
    assert _equal(dev, _run_device(eng, plan, torch.from_numpy(plan.pack(samples)).cuda()))
    if not eng.dims.signal_out:
        assert K.bits_equal(dev[0], want[0]) and (dev[1] is None or K.bits_equal(dev[1], want[1]))
    else:  # (the host form downloads an arena it cleared; the device form's is the caller's: the utterances' samples are what both write)
        n = ceng.load_library().ctu_plan_out_samples(plan._h)
        for i in range(plan.n_utt):
            a, b = int(plan.sample_off[i]), int(plan.sample_off[i]) + int(n[i])
            assert np.array_equal(dev[0][a:b], want[0][a:b])
    for shift in (1, 2, 4):   # arenas at 2, 4 and 8 bytes past a 16-byte boundary
        _unpack(eng, plan, buf, off, fmt, stride, samples, shift=shift)
    # another junk filling of the elements nobody names
    buf2, off2, samples2 = _lay(ns, fmt, stride, fs, seed=1, pick=5)
    assert np.array_equal(off2, off) and not np.array_equal(buf2, buf) and _same(samples2, samples)
    assert _equal(_run_host(eng, plan, samples, buf2, off, fmt, stride), want)
    # the conveniences cut the same results per utterance
    if eng.dims.signal_out:
        assert _same(eng.enhance_wire(buf, off, ns, fmt=fmt, stride=stride), eng.enhance(samples))
    else:
        assert _same(eng.extract_wire(buf, off, ns, fmt=fmt, stride=stride), eng.extract(samples))
    plan.close()


@pytest.mark.parametrize("name,fmt,stride", [("c2", "alaw", 1), ("c4", "s16_swapped", 2), ("m44", "mulaw", 3)])
def test_ranges_on_two_streams(name, fmt, stride, monkeypatch):
    """The host form cut into utterance ranges (CTU_HOST_CHUNKS, as the 32 MiB rule cuts a large page-locked batch): every range uploads
    the covering range of its own utterances - here of descending, overlapping ones - and the rows are those of the run in one range."""
    eng = _engine(name)
    _, fs, most, _ = ENGINES[name]
    ns = _lengths(eng.dims, most)
    buf, off, samples = _lay(ns, fmt, stride, fs)
    plan = eng.plan(ns)
    want = _run_host(eng, plan, samples)
    for chunks in ("3", "8"):
        monkeypatch.setenv("CTU_HOST_CHUNKS", chunks)
        assert _equal(_run_host(eng, plan, samples, buf, off, fmt, stride), want), chunks
    pin = ceng.host_alloc(buf.shape, buf.dtype)
    pin[...] = buf
    rows = ceng.host_alloc((plan.total_frames, eng.dims.row_floats), np.float32)
    got = eng.run_wire_host(plan, pin, off, fmt=fmt, stride=stride, want_vad=True, rows_out=rows)
    assert _equal(got, want)
    monkeypatch.delenv("CTU_HOST_CHUNKS")
    plan.close()


def test_no_samples_not_looked_at():
    """An utterance of 0 samples is not looked at: its elem_off is -1.  (An engine whose hop is its window: elsewhere no plan holds one.)"""
    eng = _engine("hop")
    d = eng.dims
    assert d.window == d.wshift
    ns = [d.window * 3 + 1, 0, d.window, 0]
    buf, off, samples = _lay(ns, "alaw", 2, 16000)
    assert off[1] == -1 and off[3] == -1
    plan = eng.plan(ns)
    want = _run_host(eng, plan, samples)
    assert _equal(_run_host(eng, plan, samples, buf, off, "alaw", 2), want)
    assert K.bits_equal(_run_device(eng, plan, _unpack(eng, plan, buf, off, "alaw", 2, samples))[0], want[0])
    plan.close()
    empty = eng.plan([0, 0])   # nothing to read: no buffer needed
    assert eng.run_wire_host(empty, np.zeros(0, np.int16), [-1, -1]).shape[0] == 0
    empty.close()


def test_all_lengths_and_residues():
    """Every residue of elem_off (mod 16 bytes) and every tail length r, all formats, contiguous and strided, on one engine: the unpack alone."""
    eng = _engine("c2")
    ns = _lengths(eng.dims, 6)
    plan = eng.plan(ns)
    for fmt in ("s16", "s16_swapped", "alaw", "mulaw"):
        for stride in (1, 2, 3):
            buf, off, samples = _lay(ns, fmt, stride, 16000)
            _unpack(eng, plan, buf, off, fmt, stride, samples, shift=3 if stride == 2 else 0)
    plan.close()


def test_fwss_chain_order_and_reset():
    """hwss / fwss / 2fwss: a list is one chain, a run leaves its last spectrum to the next; the wire run is the plain run in that too."""
    eng = _engine("fwss")
    d = eng.dims
    ns = [d.window + 30 * d.wshift + 1, d.window + 20 * d.wshift + 7, d.window + 25 * d.wshift + 15]
    x = [synth_utt(40 + i, n) for i, n in enumerate(ns)]
    codes = [_g711_speech("alaw", u) for u in x]
    off = np.array([ns[1] + ns[2] + 17 + 3, ns[2] + 17, 1], np.int64)   # descending, junk between
    buf = _junk(np.uint8, int(off[0]) + ns[0], 9)
    for c, o in zip(codes, off):
        buf[o:o + c.size] = c
    samples = [ceng.wire_expand(buf, int(o), int(n), fmt="alaw") for o, n in zip(off, ns)]
    eng.reset_chain()
    a1, a2 = eng.extract(samples), eng.extract(samples)
    assert not _same(a1, a2), "the second run of the chain starts from the first one's state"
    eng.reset_chain()
    b1, b2 = eng.extract_wire(buf, off, ns, fmt="alaw"), eng.extract_wire(buf, off, ns, fmt="alaw")
    assert _same(b1, a1) and _same(b2, a2)
    eng.reset_chain()
    assert _same(eng.extract_wire(buf, off, ns, fmt="alaw"), a1)
    # list order is chain order: the same files the other way round are another run, and the wire run follows
    eng.reset_chain()
    r1 = eng.extract(samples[::-1])
    eng.reset_chain()
    assert _same(eng.extract_wire(buf, off[::-1].copy(), ns[::-1], fmt="alaw"), r1)


def test_fwss_long_files_in_two_runs():
    """The chain over files of many tiles, as a list read in two batches runs it: swapped stereo files of 180 000, 170 000 and 60 000
    samples a channel, the first two files in one run and the third in the next, against the plain run of the six channels at once."""
    eng = _engine("fwss")
    files = [np.stack([synth_utt(300 + 10 * i + c, n) for c in range(2)], axis=1) for i, n in enumerate((180000, 170000, 60000))]
    samples = [f[:, c].copy() for f in files for c in range(2)]
    buf = np.concatenate([f.reshape(-1) for f in files]).byteswap()
    ns = [len(u) for u in samples]
    off = np.array([2 * sum(len(f) for f in files[:i]) + c for i in range(3) for c in range(2)], np.int64)
    eng.reset_chain()
    want = eng.extract(samples)
    eng.reset_chain()
    got = (eng.extract_wire(buf, off[:4], ns[:4], fmt="s16_swapped", stride=2) + eng.extract_wire(buf, off[4:], ns[4:], fmt="s16_swapped", stride=2))
    assert _same(got, want)
    eng.reset_chain()
    assert _same(eng.extract_wire(buf, off, ns, fmt="s16_swapped", stride=2), want)


def test_extract_interleaved():
    """A [samples, channels] block: one utterance per channel, in channel order."""
    eng = _engine("m8")
    n = eng.dims.window + 11 * eng.dims.wshift + 3
    frames = np.stack([synth_utt(60 + c, n, fs=8000) for c in range(3)], axis=1)
    frames = np.ascontiguousarray(frames)
    want = eng.extract([frames[:, c].copy() for c in range(3)])
    assert _same(eng.extract_interleaved(frames), want)
    assert _same(eng.extract_interleaved(frames.byteswap(), fmt="s16_swapped"), want)


# ---- refusals: CTU_ERR_INPUT, the words, and nothing written
def _refusal_cases(ns):
    big = 2 ** 62
    return [
        ("format", dict(fmt=7), "unknown format"),
        ("stride", dict(stride=0), "stride below 1"),
        ("negative", dict(off=1, value=-1), "negative element offset"),
        ("past int64", dict(off=1, value=2 ** 63 - 5), "past int64_t"),
        ("past int64 by the stride", dict(off=1, value=big, stride=2 ** 31 - 1), "past int64_t"),
        ("odd address", dict(odd=True), "2-byte aligned"),
        ("null buffer", dict(null=True), "null buffer"),
    ]


def test_refusals():
    import torch
    L = ceng.load_library()
    eng = _engine("c2")
    d = eng.dims
    ns = np.array([d.window + 3 * d.wshift, d.window], np.int64)
    plan = eng.plan(ns)
    buf = synth_utt(3, int(ns.sum()) + 64)
    dev = torch.from_numpy(buf).cuda()
    good = np.array([0, ns[0]], np.int64)
    pa, pb = K.POISON["int16"]
    fa, fb = K.POISON["float32"]

    def poisoned():
        pcm = K.guarded(plan.total_samples, torch.int16, K.GUARD_SAMPLES, pa)
        rows = np.full((plan.total_frames, d.row_floats), fa, np.uint32).view(np.float32)
        return pcm, rows

    def untouched(pcm, rows):
        torch.cuda.synchronize()
        assert K.guards_intact(pcm[0], pcm[1], pa) and bool((pcm[1] == pa).all()), "d_pcm written behind a refusal"
        assert bool(np.all(rows.view(np.uint32) == fa)), "h_rows written behind a refusal"

    for what, c, words in _refusal_cases(ns):
        off = good.copy()
        if "off" in c:
            off[c["off"]] = c["value"]
        w = ceng.WireLayout(c.get("fmt", 0), c.get("stride", 1))
        d_in = None if c.get("null") else dev.data_ptr() + (1 if c.get("odd") else 0)
        h_in = None if c.get("null") else buf.ctypes.data + (1 if c.get("odd") else 0)
        pcm, rows = poisoned()
        per = np.full(2, -7, np.int64)
        rc = L.ctu_plan_unpack_wire(eng._h, plan._h, d_in, off.ctypes.data, ctypes.byref(w), pcm[1].data_ptr(), None)
        assert rc == ceng.CTU_ERR_INPUT and words in L.ctu_last_error(eng._h).decode(), (what, L.ctu_last_error(eng._h))
        rc = L.ctu_engine_run_wire_host(eng._h, plan._h, h_in, off.ctypes.data, ctypes.byref(w), rows.ctypes.data, None, per.ctypes.data)
        assert rc == ceng.CTU_ERR_INPUT and words in L.ctu_last_error(eng._h).decode(), (what, L.ctu_last_error(eng._h))
        assert (per == -7).all(), what
        untouched(pcm, rows)
    # a NULL layout
    pcm, rows = poisoned()
    assert L.ctu_plan_unpack_wire(eng._h, plan._h, dev.data_ptr(), good.ctypes.data, None, pcm[1].data_ptr(), None) == ceng.CTU_ERR_INPUT
    assert "null layout" in L.ctu_last_error(eng._h).decode()
    assert L.ctu_engine_run_wire_host(eng._h, plan._h, buf.ctypes.data, good.ctypes.data, None, rows.ctypes.data, None, None) == ceng.CTU_ERR_INPUT
    assert "null layout" in L.ctu_last_error(eng._h).decode()
    # a plan of another engine
    other = _engine("m8")
    w = ceng.WireLayout(0, 1)
    assert L.ctu_plan_unpack_wire(other._h, plan._h, dev.data_ptr(), good.ctypes.data, ctypes.byref(w), pcm[1].data_ptr(), None) == ceng.CTU_ERR_INPUT
    assert "plan of another engine" in L.ctu_last_error(other._h).decode()
    assert L.ctu_engine_run_wire_host(other._h, plan._h, buf.ctypes.data, good.ctypes.data, ctypes.byref(w), rows.ctypes.data, None, None) == ceng.CTU_ERR_INPUT
    assert "plan of another engine" in L.ctu_last_error(other._h).decode()
    # the wrong family of call for the engine
    out = np.full(plan.total_samples, pa, np.int16)
    assert L.ctu_engine_run_signal_wire_host(eng._h, plan._h, buf.ctypes.data, good.ctypes.data, ctypes.byref(w), out.ctypes.data) == ceng.CTU_ERR_INPUT
    assert "needs -format_out raw|wave" in L.ctu_last_error(eng._h).decode() and bool((out == pa).all())
    untouched(pcm, rows)
    sig = _engine("sig")
    splan = sig.plan(ns)
    # the speech form refuses the same table, with h_out still poison behind it
    for what, c, words in _refusal_cases(ns):
        off = good.copy()
        if "off" in c:
            off[c["off"]] = c["value"]
        lay = ceng.WireLayout(c.get("fmt", 0), c.get("stride", 1))
        h_in = None if c.get("null") else buf.ctypes.data + (1 if c.get("odd") else 0)
        rc = L.ctu_engine_run_signal_wire_host(sig._h, splan._h, h_in, off.ctypes.data, ctypes.byref(lay), out.ctypes.data)
        assert rc == ceng.CTU_ERR_INPUT and words in L.ctu_last_error(sig._h).decode(), (what, L.ctu_last_error(sig._h))
        assert bool((out == pa).all()), what
    assert L.ctu_engine_run_signal_wire_host(sig._h, splan._h, buf.ctypes.data, good.ctypes.data, None, out.ctypes.data) == ceng.CTU_ERR_INPUT
    assert "null layout" in L.ctu_last_error(sig._h).decode() and bool((out == pa).all())
    assert L.ctu_engine_run_signal_wire_host(sig._h, plan._h, buf.ctypes.data, good.ctypes.data, ctypes.byref(w), out.ctypes.data) == ceng.CTU_ERR_INPUT
    assert "plan of another engine" in L.ctu_last_error(sig._h).decode() and bool((out == pa).all())
    assert L.ctu_engine_run_wire_host(sig._h, splan._h, buf.ctypes.data, good.ctypes.data, ctypes.byref(w), rows.ctypes.data, None, None) == ceng.CTU_ERR_INPUT
    assert "use ctu_engine_run_signal_wire_host" in L.ctu_last_error(sig._h).decode()
    untouched(pcm, rows)
    splan.close()
    # an engine over feature files
    htk = ceng.Engine(HTK + "-nfeacoefs 13 -fea_delta d_a".split())
    hplan = htk.plan([8, 9])
    hoff = np.zeros(2, np.int64)
    for rc in (L.ctu_plan_unpack_wire(htk._h, hplan._h, dev.data_ptr(), hoff.ctypes.data, ctypes.byref(w), pcm[1].data_ptr(), None),
               L.ctu_engine_run_wire_host(htk._h, hplan._h, buf.ctypes.data, hoff.ctypes.data, ctypes.byref(w), rows.ctypes.data, None, None),
               L.ctu_engine_run_signal_wire_host(htk._h, hplan._h, buf.ctypes.data, hoff.ctypes.data, ctypes.byref(w), out.ctypes.data)):
        assert rc == ceng.CTU_ERR_INPUT and "use ctu_engine_run_rows" in L.ctu_last_error(htk._h).decode()
    untouched(pcm, rows)
    assert bool((out == pa).all())
    hplan.close()
    htk.close()
    # the Python layer passes a refusal on
    with pytest.raises(CtuError, match="negative element offset"):
        eng.extract_wire(buf, [0, -3], [int(ns[0]), int(ns[1])])
    # ... and the plan still runs
    rows = eng.run_wire_host(plan, buf, good)
    assert K.bits_equal(rows, eng.run_host(plan, plan.pack([buf[:ns[0]], buf[ns[0]:ns[0] + ns[1]]])))
    plan.close()
