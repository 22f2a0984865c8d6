"""Stream sets with large-transform state on the GPU (Engine.streams(..., large_state=True)): -nr_mode exten and speech output on
1024 .. 4096-point frames behind pushed samples give the offline run's rows and samples, with exten's estimate (wave1k_kernel /
bigfft_kernel<..., XS>) and the overlap-add's tail (up to 4095 sums: stream_ola_big_kernel) kept per stream between the pushes.

Bounds.  Bit identity where DESIGN.md section 4.10 derives it: pushes that end a multiple of eight frames into the file, the estimate's
floats through memory as they stand, a sample's partial sum continued in frame order.  Elsewhere the bounds the project holds the
offline run to at the same configurations: _assert_rows (tests/test_gpu_parity.py: test_exten_at_1024_points,
test_exten_and_vad_at_2048_and_4096_points) for the rows; 1 LSB against the offline run and (2 LSB, mean 0.3) against the oracle
(test_enhancement_output_above_512_points) for the samples."""
import numpy as np
import pytest

from ctucopy_amd import CtuError
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_gpu_parity import _assert_rows
from tests.test_streams import _schedule, _signal
from tests.test_streams_nr import _eights, _stream as _stream_rows
from tests.test_streams_signal import _eights as _eights_signal, _lsb, _stream as _stream_signal
from tests.util import C2, synth_utt

pytestmark = pytest.mark.gpu

EXTEN = ["-nr_mode", "exten"]
FEAT = {
    "1024": C2 + ["-w", "40", "-s", "10"] + EXTEN,
    "2048": "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97".split() + EXTEN,
    "4096": "-fs 48000 -format_in raw -format_out htk -preset mfcc -preem 0.97 -w 64 -s 16".split() + EXTEN,
}
SPEECH = {
    "1024_plain": "-fs 16000 -format_in raw -format_out raw -w 40 -s 20".split(),
    "2048_exten": "-fs 44100 -format_in raw -format_out raw -w 24 -s 12.5 -nr_mode exten".split(),
    "2048_odd_window": "-fs 44100 -format_in raw -format_out raw -w 25 -s 10 -nr_mode exten".split(),
    "4096_plain": "-fs 48000 -format_in raw -format_out raw -w 64 -s 16".split(),
    "4096_exten": "-fs 48000 -format_in raw -format_out raw -w 64 -s 16 -nr_mode exten".split(),
}
FRAMES = {"4096": 40, "4096_plain": 40, "4096_exten": 40}
KERNEL = {"1024": "wave1k_kernel", "2048": "bigfft_kernel<8>", "4096": "bigfft_kernel<16>"}


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


_cache = {}


def _feat(Engine, name):
    """(configuration, engine, signal, the offline run's rows) of a feature configuration, made once for the module and left unchanged."""
    if name not in _cache:
        cfg = FEAT[name]
        eng = Engine(cfg)
        assert eng.kernel_name() == KERNEL[name]
        x = _signal(eng, FRAMES.get(name, 96))
        off = eng.extract([x])[0]
        assert off.shape[0] == FRAMES.get(name, 96)
        off.setflags(write=False)
        _cache[name] = (cfg, eng, x, off)
    return _cache[name]


def _speech(Engine, name):
    """(configuration, engine, signal, the offline run's samples) of a speech configuration, likewise."""
    if name not in _cache:
        cfg = SPEECH[name]
        eng = Engine(cfg)
        assert eng.dims.signal_out == 1 and eng.dims.window > 512
        frames = FRAMES.get(name, 96)
        x = _signal(eng, frames)
        off = eng.enhance([x])[0]
        assert off.size == frames * eng.dims.wshift + eng.dims.window - eng.dims.wshift
        off.setflags(write=False)
        _cache[name] = (cfg, eng, x, off)
    return _cache[name]


def _other(eng, frames, seed):
    """A signal of `frames` frames and half a hop that differs from every other seed's, at any sampling rate."""
    d = eng.dims
    return synth_utt(seed, d.window + (frames - 1) * d.wshift + d.wshift // 2, fs=d.fs)


def _fset(eng, n, max_push, row_state=False):
    return eng.streams(n, max_push, row_state=row_state, nr_state=True, large_state=True)


def _sset(eng, cfg, n, max_push):
    return eng.streams(n, max_push, nr_state="exten" in cfg, signal_state=True, large_state=True)


# ---- features behind exten


@pytest.mark.parametrize("name", list(FEAT))
def test_pushes_of_eight_hops_are_the_offline_rows_bit_for_bit(Engine, name):
    cfg, eng, x, off = _feat(Engine, name)
    w, s = eng.dims.window, eng.dims.wshift
    st = _fset(eng, 2, w + 8 * s)
    got = _stream_rows(eng, st, 1, x, _eights(eng, x), cfg)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("name", list(FEAT))
def test_arbitrary_chunking_agrees_with_the_oracle(Engine, name):
    """Largest |streamed - offline| / max(|offline|, 1) measured on gfx950: 0 at all three sizes (Large-transform
    state) - the large-transform kernels take a frame at a time, so how a push cuts the file changes no instruction a frame runs through -
    and so equality is asserted beside the oracle bound."""
    cfg, eng, x, off = _feat(Engine, name)
    w, s = eng.dims.window, eng.dims.wshift
    st = _fset(eng, 1, max(w, 17 * s))
    got = _stream_rows(eng, st, 0, x, _schedule(eng, x.size, 11), cfg)
    ref = Oracle(cfg).process(x)
    assert got.shape == ref.shape == off.shape and np.isfinite(got).all()
    print("large exten streamed vs offline rows, largest |difference| / max(|offline|, 1):",
          float((np.abs(got - off) / np.maximum(np.abs(off), 1.0)).max()), " ".join(cfg))
    _assert_rows(off, ref, cfg)
    _assert_rows(got, ref, cfg)
    assert np.array_equal(got, off)


@pytest.mark.parametrize("name", ["1024", "2048"])
def test_two_tiles_in_one_push_keep_the_estimate_in_registers_across_the_tile_edge(Engine, name):
    cfg, eng, x, off = _feat(Engine, name)
    w, s = eng.dims.window, eng.dims.wshift
    chunks = _eights(eng, x, first=72)   # tiles of 64 and 8 frames, then three pushes that load the estimate from memory
    assert chunks[:4] == [w + 71 * s, 8 * s, 8 * s, 8 * s] and len(chunks) == 5
    st = _fset(eng, 1, w + 71 * s)
    got = _stream_rows(eng, st, 0, x, chunks, cfg)
    eights = _stream_rows(eng, _fset(eng, 1, w + 8 * s), 0, x, _eights(eng, x), cfg)
    assert got.shape == off.shape and np.array_equal(got, eights) and np.array_equal(got, off)


@pytest.mark.parametrize("name", ["1024", "2048"])
def test_more_streams_than_chains_store_and_load_the_estimate_inside_one_chain(Engine, name):
    import torch
    cfg, eng, _, _ = _feat(Engine, name)
    w, s = eng.dims.window, eng.dims.wshift
    # bigfft_kernel walks 8 workgroup chains per CU; wave1k_kernel's wave chains are at most two workgroups of four waves per CU
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    sigs = [_other(eng, 12, 40 + k) for k in range(4)]
    assert len({x.tobytes() for x in sigs}) == 4
    off = [r[:6] for r in eng.extract(sigs)]
    st = _fset(eng, n, w + s)
    got, at = [[] for _ in range(n)], 0
    for c in (w + s, 2 * s, 2 * s):
        out = st.push({i: sigs[i % 4][at:at + c] for i in range(n)})
        at += c
        for i in range(n):
            assert out[i].shape[0] == 2
            got[i].append(out[i])
    wrong = [i for i in range(n) if not np.array_equal(np.concatenate(got[i]), off[i % 4])]
    assert not wrong, (len(wrong), wrong[:8])


@pytest.mark.parametrize("name", ["1024", "2048"])
def test_streams_in_different_phases_share_a_push_and_a_finished_stream_starts_afresh(Engine, name):
    cfg, eng, _, _ = _feat(Engine, name)
    w, s = eng.dims.window, eng.dims.wshift
    xa, xb, xc, xd1, xd2 = (_other(eng, 40, 50 + k) for k in range(5))
    assert len({v.tobytes() for v in (xa, xb, xc, xd1, xd2)}) == 5
    offl = dict(zip("abcd", eng.extract([xa, xb, xc, xd2])))
    A, B, C, D = 3, 0, 2, 1
    st = _fset(eng, 4, w + 8 * s)
    got = {A: [], B: [], C: [], D: []}
    # ahead of the push in question: B and C have had a first push, D a whole file
    first = st.push({B: xb[:w + 7 * s], C: xc[:w + 7 * s]})
    got[B].append(first[B])
    got[C].append(first[C])
    assert np.array_equal(_stream_rows(eng, st, D, xd1, _eights(eng, xd1), cfg), eng.extract([xd1])[0])
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
    for k, nm in ((A, "a"), (B, "b"), (C, "c"), (D, "d")):
        assert st.frames(k) == 40
        assert np.array_equal(np.concatenate(got[k]), offl[nm]), nm   # (D: the second file alone, from the reference's initial estimate)


def test_delta_chain_behind_exten_at_1024_points_with_row_state(Engine):
    cfg = FEAT["1024"] + ["-fea_delta", "d_a"]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 96)
    off = eng.extract([x])[0]
    st = _fset(eng, 2, w + 8 * s, row_state=True)
    got = _stream_rows(eng, st, 1, x, _eights(eng, x), cfg)
    assert got.shape == off.shape and np.array_equal(got, off)


# ---- speech


@pytest.mark.parametrize("name", list(SPEECH))
def test_pushes_of_eight_hops_are_the_offline_samples_bit_for_bit(Engine, name):
    cfg, eng, x, off = _speech(Engine, name)
    w, s = eng.dims.window, eng.dims.wshift
    st = _sset(eng, cfg, 2, w + 8 * s)
    got = _stream_signal(eng, st, 1, x, _eights_signal(eng, x))
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("name", list(SPEECH))
def test_any_chunking_is_within_one_lsb_of_the_offline_run_and_within_its_bound_of_the_oracle(Engine, name):
    cfg, eng, x, off = _speech(Engine, name)
    w, s = eng.dims.window, eng.dims.wshift
    st = _sset(eng, cfg, 1, max(w, 17 * s))
    got = _stream_signal(eng, st, 0, x, _schedule(eng, x.size, 11))
    assert got.size == off.size
    d = _lsb(got, off)
    ref = Oracle(cfg).enhance(x)
    do = _lsb(got, ref)
    print("large signal set %s: %.4f %% of the samples differ from the offline run, worst %d LSB; against the oracle max %d LSB, mean %.4f"
          % (name, 100.0 * float((d > 0).mean()), int(d.max()), int(do.max()), float(do.mean())))
    assert d.max() <= 1
    assert ref.shape == got.shape and do.max() <= 2 and do.mean() <= 0.3


@pytest.mark.parametrize("name", ["4096_plain", "4096_exten"])
def test_a_tail_longer_than_a_slice_of_the_overlap_add(Engine, name):
    """Window 3072, shift 768: the tail holds 2304 sums, more than one slice of 2048 samples.  Pushes of three frames deliver exactly
    2304 samples (a second slice wholly inside the tail), pushes of eight 6144 (slices inside, across and past it), pushes of one frame
    keep tail entries alive over three pushes: all in the same pushes of one set."""
    cfg, eng, _, _ = _speech(Engine, name)
    w, s = eng.dims.window, eng.dims.wshift
    assert (w, s) == (3072, 768) and w - s > 2048
    xs = [_other(eng, 40, 70 + k) for k in range(4)]
    assert len({x.tobytes() for x in xs}) == 4
    off = eng.enhance(xs)
    n = xs[0].size

    def hops(k):
        out = [w + (k - 1) * s]
        while sum(out) + k * s <= n:
            out.append(k * s)
        return out + [n - sum(out)]

    plans = [hops(3), hops(8), hops(1), _schedule(eng, n, 5)]
    assert all(sum(p) == n for p in plans) and plans[0][1] == 3 * s == w - s
    st = _sset(eng, cfg, 4, max(w + 7 * s, 17 * s))
    got, at = [[] for _ in range(4)], [0] * 4
    for step in range(max(len(p) for p in plans)):
        push = {k: xs[k][at[k]:at[k] + plans[k][step]] for k in range(4) if step < len(plans[k])}
        for k, r in st.push_signal(push).items():
            got[k].append(r.copy())
            at[k] += push[k].size
    for k in range(4):
        assert st.frames(k) == 40 and st.pending(k) == w - s
        got[k].append(st.finish_signal(k).copy())
        g = np.concatenate(got[k])
        d = _lsb(g, off[k])
        print("tail beyond a slice, %s, schedule %d: %.4f %% of the samples differ from the offline run, worst %d LSB" % (name, k, 100.0 * float((d > 0).mean()), int(d.max())))
        assert g.size == off[k].size and d.max() <= 1, k
    assert np.array_equal(np.concatenate(got[1]), off[1])   # eights: bit for bit
    do = _lsb(np.concatenate(got[0]), Oracle(cfg).enhance(xs[0]))
    assert do.max() <= 2 and do.mean() <= 0.3


def test_finish_delivers_the_tail_and_a_short_file_is_refused(Engine):
    cfg, eng, x, off = _speech(Engine, "2048_exten")
    w, s = eng.dims.window, eng.dims.wshift
    st = _sset(eng, cfg, 2, w + 8 * s)
    assert st.push_signal({1: x[:w - s - 1]})[1].size == 0
    with pytest.raises(CtuError, match="shorter than one frame") as ei:
        st.finish_signal(1)
    assert ei.value.code == ceng.CTU_ERR_INPUT and st.frames(1) == 0 and st.pending(1) == 0
    # a file with the first samples loaded but no frame: nothing to deliver, and no error
    assert st.push_signal({1: x[:w - 1]})[1].size == 0 and st.pending(1) == 0
    assert st.finish_signal(1).size == 0
    # the stream starts a new file: every push's count, frames and pending against ctu_streams_signal_step (_stream_signal), the
    # finish the last window - wshift samples of the offline run
    chunks = _eights_signal(eng, x)
    got = _stream_signal(eng, st, 1, x, chunks)
    assert np.array_equal(got, off) and np.array_equal(got[-(w - s):], off[-(w - s):])


def test_without_the_flag_the_sets_are_refused_with_todays_words(Engine):
    eng = _feat(Engine, "1024")[1]
    for kw in ({"nr_state": True}, {"nr_state": True, "row_state": True}):
        with pytest.raises(CtuError) as ei:
            eng.streams(2, 4000, **kw)
        assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and "-nr_mode exten on 1024-point frames" in str(ei.value)
    seng = _speech(Engine, "2048_exten")[1]
    with pytest.raises(CtuError) as ei:
        seng.streams(2, 4000, nr_state=True, signal_state=True)
    assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and "-format_out raw | wave on 2048-point frames" in str(ei.value)


def test_offline_runs_between_two_pushes_change_neither(Engine):
    cfg, eng, x, off = _feat(Engine, "2048")
    w, s = eng.dims.window, eng.dims.wshift
    st = _fset(eng, 2, w + 8 * s)
    a = st.push({1: x[:w + 7 * s]})[1]
    other = _other(eng, 70, 90)
    mid = eng.extract([other, x])
    b = st.push({1: x[w + 7 * s:w + 15 * s]})[1]
    assert np.array_equal(np.concatenate([a, b]), off[:16]) and np.array_equal(mid[1], off)
    assert np.array_equal(eng.extract([other])[0], mid[0])
    cfg, eng, x, off = _speech(Engine, "2048_exten")
    w, s = eng.dims.window, eng.dims.wshift
    st = _sset(eng, cfg, 2, w + 8 * s)
    a = st.push_signal({0: x[:w + 7 * s]})[0].copy()
    mid = eng.enhance([x])[0]
    b = st.push_signal({0: x[w + 7 * s:w + 15 * s]})[0].copy()
    assert np.array_equal(np.concatenate([a, b]), off[:16 * s]) and np.array_equal(mid, off)
