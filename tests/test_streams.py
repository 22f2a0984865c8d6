"""Streaming input on the GPU (Engine.streams): samples pushed in chunks give the rows of the offline run.

Bounds: bit identity where DESIGN.md section 4.10 derives it (every push ends a multiple of eight frames into the file; a stream's
rows do not depend on the other streams of a push), elsewhere the oracle bound of tests/test_gpu_parity.py (_assert_rows), imported."""
import numpy as np
import pytest

from ctucopy_amd import CtuError
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_gpu_parity import _assert_rows
from tests.util import C2, C3, sig, synth_utt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


C2_8K = "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97".split()


def _signal(eng, frames, seed=5):
    """`frames` frames' worth of samples and a few more that complete none."""
    d = eng.dims
    n = d.window + (frames - 1) * d.wshift + d.wshift // 2
    x = sig("CS0")
    return x[:n].copy() if n <= x.size and d.fs == 16000 else synth_utt(seed, n, fs=d.fs)


def _schedule(eng, total, seed):
    """Chunk lengths adding up to `total`: pushes of 0, 1, wshift-1, wshift and window-1 samples, pushes that complete 1, 7, 9 and 17
    frames, the rest in a seeded random order of small pushes."""
    w, s = eng.dims.window, eng.dims.wshift
    rng = np.random.default_rng(seed)
    fixed = [0, 1, s - 1, s, 0, 7 * s, 9 * s, 17 * s, s + 1]
    fixed = [w - 1] + [fixed[i] for i in rng.permutation(len(fixed))]  # (behind w - 1 samples a push of k hops completes k frames)
    out, left = [], total
    for c in fixed:
        c = min(c, left)
        out.append(c)
        left -= c
    while left:
        c = min(int(rng.integers(0, 3 * s)), left)
        out.append(c)
        left -= c
    assert sum(out) == total
    return out


def _stream(eng, st, sid, x, chunks):
    """Pushes x in `chunks` on stream sid; the rows, after checking the count of every push against the offline frame count."""
    got, at = [], 0
    for c in chunks:
        r = st.push({sid: x[at:at + c]})[sid]
        at += c
        got.append(r)
        assert sum(g.shape[0] for g in got) == max(eng.num_frames(at), 0) == st.frames(sid), (at, c)
    return np.concatenate(got) if got else np.empty((0, eng.dims.row_floats), np.float32)


@pytest.mark.parametrize("cfg", [C2, C2_8K, C2 + ["-w", "40"], "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97".split()],
                         ids=["512", "256", "1024", "2048"])
def test_pushes_of_eight_hops_are_bit_identical_to_the_offline_run(Engine, cfg):
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 96)
    off = eng.extract([x])[0]
    assert off.shape[0] == 96
    st = eng.streams(2, w + 8 * s)
    chunks = [w + 7 * s] + [8 * s] * 11 + [x.size - (w + 95 * s)]
    got = _stream(eng, st, 1, x, chunks)
    assert got.shape == off.shape and np.array_equal(got, off)
    assert st.finish(1).shape == (0, eng.dims.row_floats)
    assert st.frames(1) == 0


@pytest.mark.parametrize("cfg", [C2, C2_8K, C2 + ["-w", "40"], "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97".split()],
                         ids=["512", "256", "1024", "2048"])
def test_arbitrary_chunking_agrees_with_the_oracle(Engine, cfg):
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 96)
    st = eng.streams(1, max(w, 17 * s))
    got = _stream(eng, st, 0, x, _schedule(eng, x.size, 11))
    ref = Oracle(cfg).process(x)
    assert got.shape == ref.shape and np.isfinite(got).all()
    _assert_rows(got, ref, cfg)
    off = eng.extract([x])[0]
    print("streamed vs offline rows, largest |difference| / max(|offline|, 1):", float((np.abs(got - off) / np.maximum(np.abs(off), 1.0)).max()), " ".join(cfg))
    _assert_rows(got, off, cfg)  # "to rounding": no further than the oracle is allowed to be


def test_a_stream_s_rows_do_not_depend_on_the_other_streams(Engine):
    eng = Engine(C2)
    w, s = eng.dims.window, eng.dims.wshift
    a, b, c = _signal(eng, 70), synth_utt(8, w + 50 * s), synth_utt(9, w + 40 * s + 5)
    ca = _schedule(eng, a.size, 3)
    alone = _stream(eng, eng.streams(1, max(w, 17 * s)), 0, a, ca)
    st = eng.streams(4, max(w, 17 * s))   # A = stream 2, B = 0, C = 3; stream 1 gets nothing for a long while
    rng = np.random.default_rng(4)
    at = {0: 0, 2: 0, 3: 0}
    got = {0: [], 1: [], 2: [], 3: []}
    step = 0
    for n_a in ca:
        # A, B, A + C, B, ...: B alone between the pushes that carry A
        p = {2: a[at[2]:at[2] + n_a]}
        at[2] += n_a
        if step % 2:
            n_c = int(rng.integers(0, 4 * s))
            p[3] = c[at[3]:at[3] + n_c]
            at[3] += p[3].size
        if step == 12:
            p[1] = b[:w + 3 * s]
        for k, r in st.push(p).items():
            got[k].append(r)
        piece = b[at[0]:at[0] + int(rng.integers(0, 3 * s))]
        got[0].append(st.push({0: piece})[0])
        at[0] += piece.size
        step += 1
    assert np.array_equal(np.concatenate(got[2]), alone)
    orc = Oracle(C2)
    _assert_rows(np.concatenate(got[0]), orc.process(b[:at[0]]), C2)
    _assert_rows(np.concatenate(got[3]), orc.process(c[:at[3]]), C2)
    assert np.concatenate(got[1]).shape[0] == 4


def test_a_finished_stream_starts_a_new_file(Engine):
    eng = Engine(C2)
    w, s = eng.dims.window, eng.dims.wshift
    x, y = _signal(eng, 60), synth_utt(31, w + 44 * s + 9)
    cy = _schedule(eng, y.size, 7)
    fresh = _stream(eng, eng.streams(2, max(w, 17 * s)), 1, y, cy)
    st = eng.streams(2, max(w, 17 * s))
    _stream(eng, st, 1, x, _schedule(eng, x.size, 6))   # ends with samples in the carry that belong to no frame
    assert st.finish(1).shape[0] == 0 and st.frames(1) == 0
    again = _stream(eng, st, 1, y, cy)
    assert np.array_equal(again, fresh)
    _assert_rows(again, Oracle(C2).process(y), C2)


@pytest.mark.parametrize("cfg", [C3, C2 + ["-fea_kind", "logspec", "-fea_E", "on"], C2 + ["-fea_E", "on", "-fea_rawenergy", "on"],
                                 C2 + ["-fb_definition", "40filters", "-fea_ncepcoefs", "39"], C2 + ["-s", "10.0625"],
                                 C2_8K + ["-w", "8", "-s", "4", "-fb_definition", "1-10/10filters", "-fea_ncepcoefs", "8"]],
                         ids=["plp", "logspec_E", "rawenergy", "hires", "odd_shift", "64_points"])
def test_configurations(Engine, cfg):
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 70)
    st = eng.streams(3, max(w, 17 * s))
    got = _stream(eng, st, 2, x, _schedule(eng, x.size, 21))
    ref = Oracle(cfg).process(x)
    assert got.shape == ref.shape and np.isfinite(got).all()
    _assert_rows(got, ref, cfg)


def test_argument_errors_leave_the_set_usable(Engine):
    import ctypes
    eng = Engine(C2)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 40)
    st = eng.streams(3, w + 8 * s)
    L = ceng.load_library()
    first = st.push({0: x[:w + 7 * s]})[0]
    assert first.shape[0] == 8

    def raw_push(ids, lens, cap):
        ids = np.array(ids, dtype=np.int32)
        ns = np.array(lens, dtype=np.int64)
        bufs = [np.zeros(max(int(n), 1), dtype=np.int16) for n in lens]
        ptrs = (ctypes.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
        rows = np.zeros((64, eng.dims.row_floats), dtype=np.float32)
        cnt = np.zeros(len(bufs), dtype=np.int64)
        return L.ctu_streams_push_host(st._h, len(bufs), ids.ctypes.data, ptrs, ns.ctypes.data, rows.ctypes.data, cap, cnt.ctypes.data)

    assert raw_push([1, 1], [s, s], 64) == ceng.CTU_ERR_INPUT            # a repeated id
    assert "twice" in L.ctu_last_error(eng._h).decode()
    assert raw_push([0, 3], [s, s], 64) == ceng.CTU_ERR_INPUT            # an id outside the set
    assert raw_push([0, -1], [s, s], 64) == ceng.CTU_ERR_INPUT
    assert raw_push([0], [w + 8 * s + 1], 64) == ceng.CTU_ERR_INPUT      # above max_push_samples
    assert raw_push([0, 1], [8 * s, w + 7 * s], 15) == ceng.CTU_ERR_INPUT  # 16 rows into room for 15
    with pytest.raises(CtuError) as ei:
        st.push({1: x[:s], 2: np.zeros(w + 8 * s + 1, np.int16)})
    assert ei.value.code == ceng.CTU_ERR_INPUT
    # none of them took a sample: streams 1 and 2 are empty, stream 0 goes on where it was
    assert st.frames(0) == 8 and st.frames(1) == 0 and st.frames(2) == 0
    got = [first]
    at = w + 7 * s
    for c in [8 * s, 8 * s, 8 * s, x.size - (w + 31 * s)]:
        got.append(st.push({0: x[at:at + c]})[0])
        at += c
    assert np.array_equal(np.concatenate(got), eng.extract([x])[0])
    assert st.push({1: x[:w + 7 * s]})[1].shape[0] == 8


def test_engines_that_carry_state_have_no_stream_set(Engine):
    for extra, word in ((["-nr_mode", "exten"], "-nr_mode exten"), (["-fea_delta", "d_a"], "-fea_delta"), (["-fea_Z_exp", "500"], "-fea_Z_exp")):
        eng = Engine(C2 + extra)
        with pytest.raises(CtuError) as ei:
            eng.streams(2, 1600)
        assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and word in str(ei.value)
