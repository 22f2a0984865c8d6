"""The buffer contracts of include/ctu_engine.h, per kernel family (tests/contracts.py: CASES), on the GPU: which bytes a run may
depend on and which it may write.  Every comparison is of bits; there is no tolerance and no oracle in this file.

P1 the contents of the gaps, of the padding around the arena and of a longer tensor's slack do not matter; P2 nor do an utterance's
samples behind its last frame; P3 nor the other utterances' samples; P4 nor where the utterance sits in the batch; P5 a run writes
every row, byte and sample it promises and nothing around them; P6 it leaves its input alone; P7 it depends on no earlier run."""
from collections import namedtuple

import numpy as np
import pytest

from tests import contracts as K
from tests.contracts import CASES, TARGET
from tests.util import g711_codes, lsb_noise, square_fs

pytestmark = pytest.mark.gpu

ALL = [n for n, c in CASES.items() if c.flags["kind"] != "g711"]
PCM = [n for n in ALL if CASES[n].flags["kind"] in K.PCM_KINDS]
STATELESS = [n for n in ALL if not CASES[n].flags["ss"]]   # an utterance's output depends on nothing else in the batch

Res = namedtuple("Res", "rows vad out")
Ctx = namedtuple("Ctx", "name case eng dims tile lengths utts plan base")
_ctx = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import load_library
    load_library()  # fails loudly when the HIP extension is missing


def _rows_in_utt(dims, seed, T):
    """A feature file's payload: T rows of row_floats_in floats as words in the byte order -endian_in names."""
    f = np.random.default_rng(seed).normal(0, 3, (T, dims.row_floats_in)).astype(np.float32)
    return f.reshape(-1).view(np.uint32).astype(">u4" if dims.swap_in else "<u4").view(np.uint32)


def _utts(case, dims, lengths, seed0=100):
    if dims.rows_in:
        return [_rows_in_utt(dims, seed0 + i, int(T)) for i, T in enumerate(lengths)]
    return K.batch_utts(lengths, case.flags["fs"], seed0)


def _length(dims, u):
    return len(u) // dims.row_floats_in if dims.rows_in else len(u)


WORDS = {"zeros": [0], "rails": [0x7FC00000, 0x7F800000, 0xFFFFFFFF, 0xFF800001]}   # NaN, inf, all ones, a signalling NaN


def _arena(c, plan, utts, fill, total=None):
    """The arena of `utts` under `plan` with everything between them set by `fill`."""
    if not c.dims.rows_in:
        return K.junk_arena(plan, utts, fill, total=total)
    total = max(plan.total_samples, 1) if total is None else total
    if fill == "random":
        a = np.random.default_rng(99).integers(0, 2 ** 32, total, dtype=np.uint32)
    else:
        a = np.resize(np.array(WORDS[fill], np.uint32), total)
    for u, off in zip(utts, plan.sample_off[:-1]):
        a[off:off + len(u)] = u
    return a


def _out_samples(plan):
    from ctucopy_amd import load_library
    p = load_library().ctu_plan_out_samples(plan._h)
    return [int(p[i]) for i in range(plan.n_utt)]


def _run(c, plan, arena, rows=None, vad=None, out=None, eng=None):
    """One device run of `plan` over `arena` (numpy); the results as numpy.  The input must come back as it went in (P6)."""
    import torch
    eng = eng or c.eng
    if c.case.flags["ss"]:
        eng.reset_chain()
    dev = arena if not isinstance(arena, np.ndarray) else torch.from_numpy(arena.view(np.int32) if c.dims.rows_in else arena).cuda()
    before = dev.clone()
    r = v = o = None
    if c.dims.signal_out:
        o = eng.enhance_device(plan, dev, out=out)
    elif c.dims.rows_in:
        r = eng.run_rows_device(plan, dev, rows=rows)
    else:
        if c.dims.has_vad:
            v = vad if vad is not None else torch.zeros(max(plan.total_frames, 1), dtype=torch.uint8, device="cuda")
        r = eng.run_device(plan, dev, rows=rows, vad=v)
    torch.cuda.synchronize()
    assert K.bits_equal(dev, before), "the run changed its input"
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return Res(cpu(r), None if v is None else cpu(v)[:plan.total_frames], cpu(o))


def _take(plan, res, i):
    """Utterance i's rows, bytes and samples of a result."""
    a, b = int(plan.row_off[i]), int(plan.row_off[i + 1])
    o = int(plan.sample_off[i])
    return (None if res.rows is None else res.rows[a:b], None if res.vad is None else res.vad[a:b],
            None if res.out is None else res.out[o:o + _out_samples(plan)[i]])


def _same(x, y):
    return all((p is None and q is None) or (p is not None and q is not None and K.bits_equal(p, q)) for p, q in zip(x, y))


def _same_all(plan, a, b):
    return all(_same(_take(plan, a, i), _take(plan, b, i)) for i in range(plan.n_utt))


def ctx(name):
    """Engine, batch, plan and the run over Plan.pack's zero-filled arena of a case: made once for the module, left unchanged."""
    if name not in _ctx:
        from ctucopy_amd import Engine, config_table
        case = CASES[name]
        eng = Engine(case.cfg)
        if case.kernel is not None:
            assert eng.kernel_name().startswith(case.kernel), eng.kernel_name()
        d = eng.dims
        tile = int(config_table(CASES["c2"].cfg, "tile_frames")[0])
        lengths = K.batch_lengths(d, tile, case.flags["min_frames"])
        utts = _utts(case, d, lengths)
        plan = eng.plan(lengths)
        assert [eng.num_frames(n) for n in lengths] == K.frame_counts(tile, case.flags["min_frames"])
        c = Ctx(name, case, eng, d, tile, lengths, utts, plan, None)
        if not d.rows_in:
            lay = K.Layout(lengths)
            assert np.array_equal(lay.sample_off, plan.sample_off) and lay.total_samples == plan.total_samples
            assert np.array_equal(_arena(c, plan, utts, "zeros"), plan.pack(utts))
        base = _run(c, plan, _arena(c, plan, utts, "zeros"))
        for x in base:
            if x is not None:
                x.setflags(write=False)
        _ctx[name] = c._replace(base=base)
    return _ctx[name]


# ---- P1
@pytest.mark.parametrize("name", ALL)
def test_p1_what_lies_between_the_utterances_does_not_matter(name, monkeypatch):
    import torch
    c = ctx(name)
    for fill in ("rails", "random"):
        assert _same_all(c.plan, _run(c, c.plan, _arena(c, c.plan, c.utts, fill)), c.base), fill
    # pcm as a view into a longer tensor: junk ahead of the view, in the slack past total_samples and behind the view
    total = max(c.plan.total_samples, 1)
    longer = _arena(c, c.plan, c.utts, "rails", total=total + 1000)
    whole = torch.from_numpy(np.concatenate([longer[:64][::-1], longer, longer[:64]]).view(np.int32 if c.dims.rows_in else longer.dtype)).cuda()
    assert _same_all(c.plan, _run(c, c.plan, whole[64:64 + total + 1000]), c.base)
    if name == "c2":   # the host form in two utterance ranges: each range's arena is cut out of this one
        monkeypatch.setenv("CTU_HOST_CHUNKS", "2")
        rows = c.eng.run_host(c.plan, _arena(c, c.plan, c.utts, "random"))
        assert K.bits_equal(rows, c.base.rows)


# ---- P2
@pytest.mark.parametrize("name", [n for n in PCM if n not in K.P2_EXCLUDED])
def test_p2_samples_behind_the_last_frame_do_not_matter(name):
    c = ctx(name)
    n = c.lengths[TARGET]
    cut = K.covered(c.dims, n)
    assert cut == n - (c.dims.wshift - 1) < n
    want = _take(c.plan, c.base, TARGET)
    utts = list(c.utts)
    utts[TARGET] = np.concatenate([c.utts[TARGET][:cut], K.junk(n - cut, "rails")])
    assert _same(_take(c.plan, _run(c, c.plan, _arena(c, c.plan, utts, "zeros")), TARGET), want)
    # cut off: a plan with the shorter length
    utts[TARGET] = c.utts[TARGET][:cut]
    plan = c.eng.plan([len(u) for u in utts])
    assert plan.total_frames == c.plan.total_frames
    assert _same(_take(plan, _run(c, plan, _arena(c, plan, utts, "rails")), TARGET), want)


# ---- P3
@pytest.mark.parametrize("name", STATELESS)
def test_p3_the_neighbours_samples_do_not_matter(name):
    c = ctx(name)
    want = _take(c.plan, c.base, TARGET)
    others = [_utts(c.case, c.dims, c.lengths, seed0=300)]
    if not c.dims.rows_in:
        others += [[square_fs(n) for n in c.lengths], [lsb_noise(n) for n in c.lengths]]
    for alt in others:
        utts = [u if i == TARGET else a for i, (u, a) in enumerate(zip(c.utts, alt))]
        assert all(len(a) == len(b) for a, b in zip(utts, c.utts))
        assert _same(_take(c.plan, _run(c, c.plan, _arena(c, c.plan, utts, "zeros")), TARGET), want)


# ---- P4
@pytest.mark.parametrize("name", STATELESS)
def test_p4_the_place_in_the_batch_does_not_matter(name):
    c = ctx(name)
    want = _take(c.plan, c.base, TARGET)
    rest = [u for i, u in enumerate(c.utts) if i != TARGET]
    t = c.utts[TARGET]
    orders = {"alone": [t], "first": [t] + rest, "middle": rest[:3] + [t] + rest[3:], "last": rest + [t], "reversed": list(c.utts)[::-1]}
    for how, utts in orders.items():
        at = [i for i, u in enumerate(utts) if u is t][0]
        plan = c.eng.plan([_length(c.dims, u) for u in utts])
        for _ in range(2 if how == "reversed" else 1):
            assert _same(_take(plan, _run(c, plan, _arena(c, plan, utts, "zeros")), at), want), how


# ---- P5
def _delay(case):
    cfg = case.cfg
    return ((int(cfg[cfg.index("-vad_filter_order") + 1]) if "-vad_filter_order" in cfg else 3) - 1) // 2


@pytest.mark.parametrize("name", ALL)
def test_p5_a_run_writes_what_it_promises_and_nothing_else(name):
    import torch
    c = ctx(name)
    plan, F, D = c.plan, c.plan.total_frames, c.dims.row_floats
    arena = _arena(c, plan, c.utts, "zeros")
    got = []
    for k in range(2):
        bufs = {}
        if c.dims.signal_out:
            bufs["out"] = K.guarded((plan.total_samples,), torch.int16, K.GUARD_SAMPLES, K.POISON["int16"][k])
        else:
            bufs["rows"] = K.guarded((F, D), torch.float32, K.GUARD_ROWS, K.POISON["float32"][k])
            if c.dims.has_vad:
                bufs["vad"] = K.guarded((F,), torch.uint8, K.GUARD_BYTES, K.POISON["uint8"][k])
        res = _run(c, plan, arena, **{key: view for key, (whole, view) in bufs.items()})
        for key, (whole, view) in bufs.items():
            assert K.guards_intact(whole, view, K.POISON[K._dtype_name(view.dtype)][k]), (key, k)
        got.append(res)
    a, b = got
    frames = [int(plan.row_off[i + 1] - plan.row_off[i]) for i in range(plan.n_utt)]
    if c.dims.signal_out:
        w, u = K.written(a.out, b.out), K.untouched(a.out, b.out, *K.POISON["int16"])
        promised = np.zeros(plan.total_samples, bool)
        for i, n in enumerate(_out_samples(plan)):
            assert n == frames[i] * c.dims.wshift + c.dims.window - c.dims.wshift or frames[i] == 0
            promised[int(plan.sample_off[i]):int(plan.sample_off[i]) + n] = True
        assert np.array_equal(w, promised) and np.array_equal(u, ~promised)
        assert _same_all(plan, a, c.base)
        return
    w, u = K.written(a.rows, b.rows), K.untouched(a.rows, b.rows, *K.POISON["float32"])
    assert (w ^ u).all()   # every word is one or the other
    must = np.ones(F, bool)
    if c.dims.has_vad:
        wv, uv = K.written(a.vad, b.vad), K.untouched(a.vad, b.vad, *K.POISON["uint8"])
        assert wv.all() and not uv.any()
        for i, f in enumerate(frames):
            v = a.vad[int(plan.row_off[i]):int(plan.row_off[i + 1])]
            if f <= _delay(c.case):   # the majority filter never gets ready: neither a row nor a decision
                assert not v.any()
                must[int(plan.row_off[i]):int(plan.row_off[i + 1])] = False
            else:
                assert set(np.unique(v)) <= {ord("0"), ord("1")}
        if c.case.flags["drop"]:   # the rows rows_per_utt counts: those of speech frames
            must &= a.vad == ord("1")
            assert 0 < int(must.sum()) < F
            rows, hv, per = c.eng.run_host(plan, arena, want_vad=True)
            assert K.bits_equal(hv, a.vad)
            for i in range(plan.n_utt):
                r0, keep = int(plan.row_off[i]), must[int(plan.row_off[i]):int(plan.row_off[i + 1])]
                assert per[i] == int(keep.sum()) and K.bits_equal(rows[r0:r0 + per[i]], a.rows[r0:r0 + frames[i]][keep])
    assert w[must].all()
    assert _same_all(plan, a, c.base)


@pytest.mark.parametrize("name", [n for n in ALL if CASES[n].flags["kind"] == "cmvn"])
def test_p5_cmvn_apply_stays_in_its_columns(name):
    import torch
    from oracle.oracle import cmvn_slot_columns
    c = ctx(name)
    plan, F, D = c.plan, c.plan.total_frames, c.dims.row_floats
    cols = cmvn_slot_columns(12, 2)
    assert c.eng.cmvn_cols() == len(cols) and max(cols) < D
    outside = [k for k in range(D) if k not in cols]
    assert len(outside) == (1 if "-fea_E" in c.case.cfg else 0)
    spk, n_spk = [0, 1, 0, 1, 0, 1], 2
    whole, rows = K.guarded((F, D), torch.float32, K.GUARD_ROWS, K.POISON["float32"][0])
    _run(c, plan, _arena(c, plan, c.utts, "zeros"), rows=rows)
    assert K.bits_equal(rows, c.base.rows)
    acc = c.eng.cmvn_accumulate(plan, rows, spk, n_spk)
    mean = acc[:, :-1] / acc[:, -1:]
    var = c.eng.cmvn_accumulate(plan, rows, spk, n_spk, mean=mean)
    var = var[:, :-1] / (var[:, -1:] - 1)
    assert K.bits_equal(rows, c.base.rows)   # the statistics' passes read
    c.eng.cmvn_apply(plan, rows, spk, n_spk, mean, var)
    torch.cuda.synchronize()
    got = rows.cpu().numpy()
    assert K.guards_intact(whole, rows, K.POISON["float32"][0])
    assert K.bits_equal(got[:, outside], c.base.rows[:, outside])
    assert not K.bits_equal(got[:, cols], c.base.rows[:, cols])   # and it did apply
    # The apply works in place, and a NaN poison keeps its bits through (x - m) / v: a row too many would not show above.  Once more
    # between guards of finite values, which it would change - and the same statistics on the same rows give the same bits.
    whole, again = K.guarded((F, D), torch.float32, K.GUARD_ROWS, K.POISON["float32"][1])
    g = K.GUARD_ROWS * D
    whole[:g] = 1.5
    whole[g + F * D:] = 1.5
    again.copy_(torch.from_numpy(c.base.rows.copy()))
    c.eng.cmvn_apply(plan, again, spk, n_spk, mean, var)
    torch.cuda.synchronize()
    assert K.bits_equal(again, got)
    assert K.guards_intact(whole, again, np.float32(1.5).view(np.uint32))


@pytest.mark.parametrize("alaw", [1, 0])
@pytest.mark.parametrize("n", [1, 3, 4097])
def test_p5_g711_decode_writes_n_samples(n, alaw):
    import torch
    from ctucopy_amd import load_library
    c = ctx("c2")
    codes_h = g711_codes(n + 1)
    ref = None
    for shift in (0, 1):   # the output 64-byte aligned, and one sample further on
        outs = []
        for k in range(2):
            p = K.POISON["int16"][k]
            codes = torch.from_numpy(codes_h).cuda()
            whole, view = K.guarded((n + shift,), torch.int16, K.GUARD_SAMPLES, p)
            out = view[shift:]
            c.eng._check(load_library().ctu_decode_g711(c.eng._h, codes.data_ptr(), n, alaw, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            assert K.guards_intact(whole, view, p), (shift, k)
            assert K.bits_equal(codes, codes_h)
            outs.append(view.cpu().numpy())
        w, u = K.written(*outs), K.untouched(*outs, *K.POISON["int16"])
        assert w[shift:].all() and u[:shift].all() and not w[:shift].any()
        ref = outs[0][shift:] if ref is None else ref
        assert K.bits_equal(outs[0][shift:], ref)
    full = c.eng.decode_g711(torch.from_numpy(codes_h).cuda(), alaw=bool(alaw)).cpu().numpy()
    assert K.bits_equal(full[:n], ref)


# ---- P7
@pytest.mark.parametrize("name", ALL)
def test_p7_a_run_depends_on_no_earlier_run(name):
    from ctucopy_amd import Engine
    c = ctx(name)
    arena = _arena(c, c.plan, c.utts, "zeros")
    for _ in range(3):
        assert _same_all(c.plan, _run(c, c.plan, arena), c.base)
    t = c.utts[TARGET]
    alone = c.eng.plan([_length(c.dims, t)])
    batch1 = _run(c, c.plan, arena)
    solo = _run(c, alone, _arena(c, alone, [t], "zeros"))
    batch2 = _run(c, c.plan, arena)
    fresh = Engine(c.case.cfg)
    fplan, falone = fresh.plan(c.lengths), fresh.plan([_length(c.dims, t)])
    assert _same_all(alone, solo, _run(c, falone, _arena(c, falone, [t], "zeros"), eng=fresh))
    want = _run(c, fplan, arena, eng=fresh)
    assert _same_all(c.plan, batch1, want) and _same_all(c.plan, batch2, want) and _same_all(c.plan, want, c.base)
    fplan.close()
    falone.close()
    fresh.close()
