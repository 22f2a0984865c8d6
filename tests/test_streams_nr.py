"""Stream sets with noise state on the GPU (Engine.streams(..., nr_state=True)): -nr_mode exten behind pushed samples gives the rows
of the offline run, with the noise estimate (Navg, Yavg per bin) kept per stream between the pushes.

Bounds: bit identity where DESIGN.md section 4.10 derives it - pushes that end a multiple of eight frames into the file run the same
instruction stream over the same eight-frame steps, and the estimate's floats pass through memory as they stand - elsewhere the oracle
bound of tests/test_gpu_parity.py (_assert_rows: the exten class, 1e-3 element-wise and 1e-4 of the row's largest value), imported."""
import numpy as np
import pytest

from ctucopy_amd import CtuError, streams_rows_step
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_gpu_parity import _assert_rows
from tests.test_streams import _schedule, _signal
from tests.test_streams_rows import _chain
from tests.util import C2, C3, C4_NOVAD, sig

pytestmark = pytest.mark.gpu

EXTEN = ["-nr_mode", "exten"]
CONFIGS = [C2 + EXTEN, C4_NOVAD, C3 + EXTEN, C2 + EXTEN + ["-fea_E", "on"], C2 + EXTEN + ["-fea_delta", "d_a", "-fea_Z_exp", "500"]]
IDS = ["mfcc_exten", "c4_novad", "plp_exten", "mfcc_exten_E", "mfcc_exten_d_a_Zexp"]


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def _rows_held(cfg):
    return _chain(cfg) != (0, 0) or "-fea_Z_exp" in cfg or "-fea_Z_block" in cfg


def _set(eng, cfg, n, max_push):
    return eng.streams(n, max_push, row_state=_rows_held(cfg), nr_state=True)


def _stream(eng, st, sid, x, chunks, cfg):
    """Pushes x in `chunks` on stream sid and finishes; the rows, after checking every push's count, st.frames and st.pending against R(F)."""
    H, wmax = _chain(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    got, at = [], 0
    for c in chunks:
        got.append(st.push({sid: x[at:at + c]})[sid])
        at += c
        rows, pending = streams_rows_step(w, s, H, wmax, at)
        assert rows + pending == max(eng.num_frames(at), 0)
        assert sum(g.shape[0] for g in got) == rows == st.frames(sid) and st.pending(sid) == pending, (at, c)
    pending = st.pending(sid)
    got.append(st.finish(sid))
    assert got[-1].shape[0] == pending == H and st.frames(sid) == 0 and st.pending(sid) == 0
    return np.concatenate(got)


def _eights(eng, x, first=8):
    """A push that completes `first` frames, pushes of eight hops, the rest."""
    w, s = eng.dims.window, eng.dims.wshift
    out = [w + (first - 1) * s]
    while sum(out) + 8 * s <= x.size:
        out.append(8 * s)
    return out + [x.size - sum(out)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_pushes_of_eight_hops_are_bit_identical_to_the_offline_run(Engine, cfg):
    eng = Engine(cfg)
    x = _signal(eng, 96)
    off = eng.extract([x])[0]
    assert off.shape[0] == 96
    chunks = _eights(eng, x)
    assert chunks[:2] == [eng.dims.window + 7 * eng.dims.wshift, 8 * eng.dims.wshift] and len(chunks) == 13
    st = _set(eng, cfg, 2, eng.dims.window + 8 * eng.dims.wshift)
    got = _stream(eng, st, 1, x, chunks, cfg)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("cfg", [C2 + EXTEN, C4_NOVAD], ids=["mfcc_exten", "c4_novad"])
def test_two_tiles_in_one_push_keep_the_estimate_in_registers_across_the_tile_edge(Engine, cfg):
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 96)
    off = eng.extract([x])[0]
    chunks = _eights(eng, x, first=72)   # tiles of 64 and 8 frames, then three pushes that load the estimate from memory
    assert chunks[:4] == [w + 71 * s, 8 * s, 8 * s, 8 * s] and len(chunks) == 5
    st = _set(eng, cfg, 1, w + 71 * s)
    got = _stream(eng, st, 0, x, chunks, cfg)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_arbitrary_chunking_agrees_with_the_oracle(Engine, cfg):
    """Largest |streamed - offline| / max(|offline|, 1) measured on gfx950 is in DESIGN.md section 4.10 (Noise state)."""
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 96)
    st = _set(eng, cfg, 1, max(w, 17 * s))
    got = _stream(eng, st, 0, x, _schedule(eng, x.size, 11), cfg)
    ref = Oracle(cfg).process(x)
    off = eng.extract([x])[0]
    assert got.shape == ref.shape == off.shape and np.isfinite(got).all()
    print("exten streamed vs offline rows, largest |difference| / max(|offline|, 1):", float((np.abs(got - off) / np.maximum(np.abs(off), 1.0)).max()), " ".join(cfg))
    print("  element-wise error against the oracle: streamed", float((np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)).max()),
          "offline", float((np.abs(off - ref) / np.maximum(np.abs(ref), 1.0)).max()))
    _assert_rows(off, ref, cfg)
    _assert_rows(got, ref, cfg)


def test_more_streams_than_waves_store_and_load_the_estimate_inside_one_chain(Engine):
    import torch
    cfg = C4_NOVAD
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    n = 8 * 2 * torch.cuda.get_device_properties(0).multi_processor_count + 37   # 37 more than the chip holds waves of the front end
    sigs = [_signal(eng, 96, seed=40 + k) for k in range(4)]
    assert len({x.tobytes() for x in sigs}) == 4
    off = [r[:24] for r in eng.extract(sigs)]
    st = _set(eng, cfg, n, w + 7 * s)
    got, at = [[] for _ in range(n)], 0
    for c in (w + 7 * s, 8 * s, 8 * s):
        out = st.push({i: sigs[i % 4][at:at + c] for i in range(n)})
        at += c
        for i in range(n):
            assert out[i].shape[0] == 8
            got[i].append(out[i])
    wrong = [i for i in range(n) if not np.array_equal(np.concatenate(got[i]), off[i % 4])]
    assert not wrong, (len(wrong), wrong[:8])


def test_streams_in_different_phases_share_a_push(Engine):
    cfg = C2 + EXTEN
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    n = _signal(eng, 40).size
    xa, xb, xc, xd1, xd2 = (sig("CS0")[k * 9001:k * 9001 + n].copy() for k in range(5))   # five stretches of the bundled recording
    offl = dict(zip("abcd", eng.extract([xa, xb, xc, xd2])))
    A, B, C, D = 3, 0, 2, 1
    alone_a = _stream(eng, _set(eng, cfg, 1, w + 8 * s), 0, xa, _eights(eng, xa), cfg)
    fresh_d = _stream(eng, _set(eng, cfg, 1, w + 8 * s), 0, xd2, _eights(eng, xd2), cfg)
    st = _set(eng, cfg, 4, w + 8 * s)
    got = {A: [], B: [], C: [], D: []}
    # ahead of the push in question: B and C have had a first push, D a whole file
    first = st.push({B: xb[:w + 7 * s], C: xc[:w + 7 * s]})
    got[B].append(first[B])
    got[C].append(first[C])
    assert np.array_equal(_stream(eng, st, D, xd1, _eights(eng, xd1), cfg), eng.extract([xd1])[0])
    # the push: A starts a file, B goes on, C completes no frame, D starts its second file
    at = {A: 0, B: w + 7 * s, C: w + 7 * s, D: 0}
    sigs = {A: xa, B: xb, C: xc, D: xd2}
    step = {A: w + 7 * s, B: 8 * s, C: s // 2, D: w + 7 * s}
    out = st.push({k: sigs[k][at[k]:at[k] + step[k]] for k in (A, B, C, D)})
    assert [out[k].shape[0] for k in (A, B, C, D)] == [8, 8, 0, 8]
    for k in (A, B, C, D):
        got[k].append(out[k])
        at[k] += step[k]
    while any(at[k] < sigs[k].size for k in sigs):
        p = {k: sigs[k][at[k]:at[k] + 8 * s] for k in sigs if at[k] < sigs[k].size}
        for k, r in st.push(p).items():
            got[k].append(r)
            at[k] += p[k].size
    for k, name in ((A, "a"), (B, "b"), (C, "c"), (D, "d")):
        assert st.frames(k) == 40
        assert np.array_equal(np.concatenate(got[k]), offl[name]), name
    assert np.array_equal(np.concatenate(got[A]), alone_a)
    assert np.array_equal(np.concatenate(got[D]), fresh_d)


def test_offline_plans_between_pushes_share_nothing_with_the_set(Engine):
    """What a run covers travels with the run: a set's pushes (two tiles, a live chain, noise state) and offline plans of two other
    sizes, taken in turn on one engine, each give the rows they give alone, bit for bit."""
    cfg = C4_NOVAD
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    utts3 = [_signal(eng, 70, seed=60 + k)[:w + 69 * s] for k in range(3)]   # two tiles each
    utts1 = [_signal(eng, 10, seed=70)[:w + 9 * s]]
    plans = [(eng.plan([u.size for u in utts]), utts) for utts in (utts3, utts1)]
    assert [p.total_frames for p, _ in plans] == [210, 10]
    offline = lambda: [eng.run_host(p, p.pack(utts)).copy() for p, utts in plans]
    alone = offline()
    xs = [_signal(eng, 96, seed=80), _signal(eng, 40, seed=81), _signal(eng, 20, seed=82)]
    first = {0: w + 69 * s, 1: w + 9 * s}   # 70 frames to stream 0, 10 to stream 1; then the rest, and a third stream

    def streamed(between):
        st = _set(eng, cfg, 3, max(x.size for x in xs))
        got = [st.push({k: xs[k][:c] for k, c in first.items()})]
        assert [got[0][k].shape[0] for k in (0, 1)] == [70, 10]
        mid = between()
        got.append(st.push({k: xs[k][first.get(k, 0):] for k in (2, 0, 1)}))
        assert [got[1][k].shape[0] for k in (0, 1, 2)] == [26, 30, 20]
        got.append({k: st.finish(k) for k in range(3)})
        return got, mid

    want, _ = streamed(lambda: None)
    got, mid = streamed(offline)
    for a, b in zip(got, want):
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    for a, b in zip(mid + offline(), alone + alone):
        assert a.shape == b.shape and np.isfinite(a).all() and np.array_equal(a, b)


def test_the_flag_on_a_chain_without_noise_reduction_changes_nothing(Engine):
    eng = Engine(C2)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 40)
    chunks = _schedule(eng, x.size, 2)
    plain, at = [], 0
    st0 = eng.streams(1, max(w, 17 * s))
    for c in chunks:
        plain.append(st0.push({0: x[at:at + c]})[0])
        at += c
    st = eng.streams(1, max(w, 17 * s), nr_state=True)
    assert np.array_equal(_stream(eng, st, 0, x, chunks, C2), np.concatenate(plain))


def test_without_the_flag_exten_has_no_stream_set(Engine):
    eng = Engine(C2 + EXTEN)
    for kw in ({}, {"row_state": True}):
        with pytest.raises(CtuError) as ei:
            eng.streams(2, 1600, **kw)
        assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and "-nr_mode exten" in str(ei.value)
