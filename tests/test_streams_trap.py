"""Stream sets with trap state on the GPU (Engine.streams(..., trap_state=True)): -fea_kind trapdct behind the streamed front end gives
the rows of the offline run, row t with the push that brings frame t + half (half = (traplen - 1) / 2), the last half with finish.

Bounds: bit identity with the offline run where it launches the fp32 kernel (trapdct_mfma_kernel: more than 24 bands, more than 16
coefficients or a context of more than 113 frames; beyond 104 frames both kernels sum in compensated runs, through one device helper) and
every push ends a multiple of eight frames into the file (the log-mel rows are bit-identical then, and a row of
stream_trap_kernel depends on nothing but its own traplen log-mel rows); bit identity between two cuts of one file under the same
condition, and between a stream alone and among others always; elsewhere the oracle bound of tests/test_gpu_parity.py (_assert_rows),
imported.

Row counts follow stream_rows_out(half, half - 1, F) = F - half once F >= half + 1, none before: a file of exactly half + 1 frames
delivers row 0 with the push that completes its last frame and the other half rows with finish."""
import ctypes

import numpy as np
import pytest

from ctucopy_amd import CtuError, config_table, streams_config_check, streams_rows_step
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_gpu_parity import _assert_rows
from tests.test_streams import _schedule, _signal
from tests.test_streams import _stream as _stream_plain
from tests.util import C2, C5, synth_utt

pytestmark = pytest.mark.gpu

T31 = ["-fea_kind", "trapdct,31,8"]
F23 = ["-fb_definition", "23filters"]


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def _half(cfg):
    kind = [v for k, v in zip(cfg[:-1], cfg[1:]) if k == "-fea_kind"][-1]
    return (int(kind.split(",")[1]) - 1) // 2


def _stream(eng, st, sid, x, chunks, cfg, finish=True):
    """Pushes x in `chunks` on stream sid and finishes; the rows, after checking every push's count, st.frames and st.pending against R(F)."""
    half = _half(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    got, at = [], 0
    for c in chunks:
        got.append(st.push({sid: x[at:at + c]})[sid])
        assert got[-1].shape[0] <= max(eng.num_frames(at + c), 0) - max(eng.num_frames(at), 0)   # no more rows than frames completed
        at += c
        rows, pending = streams_rows_step(w, s, half, half - 1, at)
        assert rows + pending == max(eng.num_frames(at), 0)
        assert sum(g.shape[0] for g in got) == rows == st.frames(sid) and st.pending(sid) == pending, (at, c)
    if finish:
        pending = st.pending(sid)
        got.append(st.finish(sid))
        assert got[-1].shape[0] == pending and st.frames(sid) == 0 and st.pending(sid) == 0
    return np.concatenate(got)


def _eights(eng, x, frames=96):
    w, s = eng.dims.window, eng.dims.wshift
    return [w + 7 * s] + [8 * s] * (frames // 8 - 1) + [x.size - (w + (frames // 8 * 8 - 1) * s)]


@pytest.mark.parametrize("cfg, frames", [
    (C2 + T31, 96), (C2 + ["-w", "40"] + T31, 96),
    (C2 + ["-fea_kind", "trapdct,103,16"], 96),         # the last short size: 26 tap groups, one accumulator chain
    (C2 + ["-fea_kind", "trapdct,105,16"], 96),         # the first long size: both kernels close the accumulator every 8 taps (trap_comp_close)
    (C2 + F23 + ["-fea_kind", "trapdct,255,16"], 144),  # the largest: 64 tap groups, 32 runs
], ids=["512", "1024", "103_16", "105_16", "255_16"])
def test_pushes_of_eight_hops_are_bit_identical_to_the_offline_fp32_kernel(Engine, cfg, frames):
    eng = Engine(cfg)   # 26 bands, or a context of more than 113 frames: the offline run launches trapdct_mfma_kernel
    half = _half(cfg)
    assert config_table(cfg, "trap_path")[0] == 0
    assert streams_config_check(cfg, trap_state=True) == (ceng.CTU_OK, "", half)
    x = _signal(eng, frames)
    off = eng.extract([x])[0]
    assert off.shape == (frames, eng.dims.nbands * (8 if half == 15 else 16))
    st = eng.streams(2, eng.dims.window + 8 * eng.dims.wshift, trap_state=True)
    got = _stream(eng, st, 1, x, _eights(eng, x, frames), cfg)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("cfg, frames, kw", [
    (C5, 130, {}),
    (C2 + ["-fea_kind", "trapdct,3,2"], 100, {}),
    (C2 + F23 + ["-fea_kind", "trapdct,255,16"], 140, {}),
    (C2 + F23 + ["-fea_kind", "trapdct,105,16"], 130, {}),
    (C2 + F23 + ["-fea_kind", "trapdct,51,20"], 100, {}),
    (C2 + F23 + ["-fea_kind", "trapdct,31,5"], 100, {}),
    (C2 + ["-nr_mode", "exten"] + T31, 100, {"nr_state": True}),
    (C2 + ["-nr_mode", "exten", "-w", "40"] + T31, 100, {"nr_state": True, "large_state": True}),
], ids=["C5", "3_2", "255_16", "105_16", "51_20", "31_5", "exten_31_8", "exten_1024_31_8"])
def test_arbitrary_chunking_agrees_with_the_oracle(Engine, cfg, frames, kw):
    """C5: traplen 101, 23 bands.  3,2: half 1, the smallest.  255,16: half 127, 64 tap groups - only 13 of 140 rows leave before finish.
    51,20: two row blocks.  31,5: D = 115, the scalar store path.  exten: the noise state beside the trap state, at 512 and 1024 points.
    A padded tap that read a row nobody wrote would show here as a non-finite value.

    Contexts of more than 104 frames (more tap groups than the short instantiations have) run the compensated form: 105_16 is the
    first such size (27 tap groups: thirteen closed runs of two and a last one of one), 255_16 the largest (32 runs).  With one fp32
    accumulator chain over its 255 taps 255_16 was 1.914e-4 from the oracle on this input, outside the bound of 1e-4: partial sums in the
    hundreds for a result below one.  The same log-mel rows contracted in float64 are 4.6e-5 from it.  Engine.extract sums the same way
    at these sizes (tests/test_trapdct_shapes.py holds it to the same bound; the identity test above to the streamed rows bit for bit)."""
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, frames)
    st = eng.streams(1, max(w, 17 * s), trap_state=True, **kw)
    got = _stream(eng, st, 0, x, _schedule(eng, x.size, 11), cfg)
    ref = Oracle(cfg).process(x)
    assert got.shape == ref.shape and ref.shape[0] == frames and np.isfinite(got).all()
    _assert_rows(got, ref, cfg)


def test_streamed_fp32_rows_against_the_offline_16_bit_split_kernel(Engine):
    """C5 offline runs trapdct_split16_kernel (two fp16 terms per operand), the stream the exact-fp32 contraction: the same rows to the
    oracle bound, not bit for bit."""
    eng = Engine(C5)
    x = _signal(eng, 130)
    off = eng.extract([x])[0]
    st = eng.streams(1, eng.dims.window + 8 * eng.dims.wshift, trap_state=True)
    got = _stream(eng, st, 0, x, _eights(eng, x, 130), C5)
    assert got.shape == off.shape == (130, 23 * 16) and np.isfinite(got).all()
    print("C5 streamed (fp32 MFMA) vs offline (fp16 split), largest |difference| / max(|offline|, 1):",
          float((np.abs(got - off) / np.maximum(np.abs(off), 1.0)).max()), " largest |difference|:", float(np.abs(got - off).max()))
    _assert_rows(got, off, C5)
    _assert_rows(got, Oracle(C5).process(x), C5)


def test_a_stream_s_rows_do_not_depend_on_the_other_streams_or_on_the_file_before(Engine):
    cfg = C2 + T31
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    mp = max(w, 17 * s)
    a, b, c = _signal(eng, 70), synth_utt(8, w + 140 * s), synth_utt(9, w + 60 * s + 5)
    ca = _schedule(eng, a.size, 3)
    alone = _stream(eng, eng.streams(1, mp, trap_state=True), 0, a, ca, cfg)
    st = eng.streams(4, mp, trap_state=True)   # A = stream 2, B = 0, C = 3
    rng = np.random.default_rng(4)
    at = {0: 0, 3: 0}
    got = {0: [], 2: [], 3: []}
    pos, shared = 0, 0
    for step, n_a in enumerate(ca):
        # B, A and - every other step - C in one push: B and C at rhythms of their own
        piece = b[at[0]:at[0] + int(rng.integers(2 * s, 4 * s))]
        p = {0: piece, 2: a[pos:pos + n_a]}
        at[0] += piece.size
        pos += n_a
        if step % 2:
            n_c = int(rng.integers(0, 4 * s))
            p[3] = c[at[3]:at[3] + n_c]
            at[3] += p[3].size
        out = st.push(p)
        for k, r in out.items():
            got[k].append(r)
        # the first MFMA column group of the push holds rows of three streams
        counts = [out[k].shape[0] for k in p]
        shared += len(counts) == 3 and min(counts) > 0 and counts[0] + counts[1] < 16
        if step == 9:   # B's file ends while A and C are under way; B starts another
            got[0].append(st.finish(0))
            _assert_rows(np.concatenate(got[0]), Oracle(cfg).process(b[:at[0]]), cfg)
            b, at[0], got[0] = b[at[0]:], 0, []
    assert shared >= 2, shared
    got[2].append(st.finish(2))
    assert np.array_equal(np.concatenate(got[2]), alone)
    while at[3] < c.size:   # the rest of C, so that its file is long enough to have rows
        got[3].append(st.push({3: c[at[3]:at[3] + mp]})[3])
        at[3] += mp
    got[3].append(st.finish(3))
    _assert_rows(np.concatenate(got[3]), Oracle(cfg).process(c), cfg)
    # a second file on stream 2: the histories were reset
    assert np.array_equal(_stream(eng, st, 2, a, ca, cfg), alone)


def test_short_files(Engine):
    cfg = C2 + T31
    half = 15
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    st = eng.streams(2, w + 8 * s, trap_state=True)
    D = eng.dims.row_floats
    # no frames at all: nothing, and no error
    assert st.finish(0).shape == (0, D)
    assert st.push({0: np.zeros(0, np.int16)})[0].shape[0] == 0 and st.finish(0).shape == (0, D)
    # exactly half + 1 frames, a window and then hop by hop: row 0 with the last frame, the other half rows with finish
    x = _signal(eng, half + 1)
    pieces = [x[:w]] + [x[w + k * s:w + (k + 1) * s] for k in range(half)] + [x[w + half * s:]]
    rows = [st.push({0: p})[0] for p in pieces]
    assert [r.shape[0] for r in rows] == [0] * half + [1, 0]
    assert st.frames(0) == 1 and st.pending(0) == half
    rows.append(st.finish(0))
    got = np.concatenate(rows)
    ref = Oracle(cfg).process(x)
    assert got.shape == ref.shape == (half + 1, D) and np.isfinite(got).all()
    _assert_rows(got, ref, cfg)
    # half frames: the offline plan's refusal, in its words; the stream starts over clean
    y = _signal(eng, 40)
    chunks = _schedule(eng, y.size, 5)
    fresh = _stream(eng, eng.streams(1, max(w, 17 * s), trap_state=True), 0, y, chunks, cfg)
    st = eng.streams(1, max(w, 17 * s), trap_state=True)
    assert st.push({0: _signal(eng, half)})[0].shape[0] == 0 and st.pending(0) == half
    with pytest.raises(CtuError) as ei:
        st.finish(0)
    assert ei.value.code == ceng.CTU_ERR_INPUT and "trapdct on fewer than (traplen+1)/2 frames" in str(ei.value)
    assert st.frames(0) == 0 and st.pending(0) == 0
    assert np.array_equal(_stream(eng, st, 0, y, chunks, cfg), fresh)


def test_a_push_larger_than_the_history(Engine):
    """48 frames (3 half = 45 and the next multiple of eight) in one push behind three small ones: both cuts end every push a multiple of
    eight frames into the file, so they agree bit for bit - and with the offline run."""
    cfg = C2 + T31
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 96)
    big = [w + 7 * s, 8 * s, 8 * s, 48 * s, 8 * s, 8 * s, x.size - (w + 87 * s)]
    got = _stream(eng, eng.streams(1, w + 48 * s, trap_state=True), 0, x, big, cfg)
    small = _stream(eng, eng.streams(1, w + 8 * s, trap_state=True), 0, x, _eights(eng, x), cfg)
    assert got.shape == small.shape == (96, 26 * 8)
    assert np.array_equal(got, small) and np.array_equal(got, eng.extract([x])[0])


def test_rows_that_do_not_fit_are_refused_before_anything_changes(Engine):
    cfg = C2 + T31
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 48)
    st = eng.streams(2, w + 24 * s, trap_state=True)
    L = ceng.load_library()
    first = st.push({0: x[:w + 23 * s]})[0]
    assert first.shape[0] == 9 and st.pending(0) == 15   # 24 frames

    def raw_push(piece, cap):
        ids = np.array([0], dtype=np.int32)
        ns = np.array([piece.size], dtype=np.int64)
        buf = np.ascontiguousarray(piece)
        ptrs = (ctypes.c_void_p * 1)(buf.ctypes.data)
        rows = np.zeros((64, eng.dims.row_floats), dtype=np.float32)
        cnt = np.zeros(1, dtype=np.int64)
        return L.ctu_streams_push_host(st._h, 1, ids.ctypes.data, ptrs, ns.ctypes.data, rows.ctypes.data, cap, cnt.ctypes.data)

    assert raw_push(x[w + 23 * s:w + 31 * s], 7) == ceng.CTU_ERR_INPUT   # 8 rows into room for 7
    assert "rows_capacity" in L.ctu_last_error(eng._h).decode()
    rows = np.zeros((14, eng.dims.row_floats), dtype=np.float32)
    cnt = ctypes.c_int64(-1)
    assert L.ctu_streams_finish_host(st._h, 0, rows.ctypes.data, 14, ctypes.byref(cnt)) == ceng.CTU_ERR_INPUT   # 15 held back, room for 14
    assert st.frames(0) == 9 and st.pending(0) == 15
    got, at = [first], w + 23 * s
    for c in [8 * s, 8 * s, x.size - (w + 39 * s)]:
        got.append(st.push({0: x[at:at + c]})[0])
        at += c
    got.append(st.finish(0))
    assert np.array_equal(np.concatenate(got), eng.extract([x])[0])


def test_the_flag_on_another_feature_kind_changes_no_row(Engine):
    eng = Engine(C2)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 40)
    chunks = _schedule(eng, x.size, 2)
    assert streams_config_check(C2, trap_state=True) == (ceng.CTU_OK, "", 0)
    plain = _stream_plain(eng, eng.streams(1, max(w, 17 * s)), 0, x, chunks)
    st = eng.streams(1, max(w, 17 * s), trap_state=True)
    flagged = _stream_plain(eng, st, 0, x, chunks)   # (its count checks: every frame's row leaves with it)
    assert plain.shape[0] == 40 and np.array_equal(flagged, plain)
    assert st.finish(0).shape == (0, eng.dims.row_floats)
