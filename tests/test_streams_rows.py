"""Stream sets with row state on the GPU (Engine.streams(..., row_state=True)): delta chains, stacking and CMS behind the streamed
front end give the rows of the offline run, the ones within the halo of the newest frame with a later push or with finish.

Bounds: bit identity where DESIGN.md section 4.10 derives it (pushes that end a multiple of eight frames into the file make the base
rows bit-identical; block 0, E and both CMS forms are copies or explicitly rounded arithmetic; delta windows of 1 and 2 multiply by 1
and 2 only), elsewhere the oracle bound of tests/test_gpu_parity.py (_assert_rows), imported."""
import numpy as np
import pytest

from ctucopy_amd import CtuError, streams_config_check, streams_rows_step
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_gpu_parity import _assert_rows
from tests.test_streams import C2_8K, _schedule, _signal
from tests.util import C2, C3, synth_utt

pytestmark = pytest.mark.gpu

DA = ["-fea_delta", "d_a"]
DAT312 = ["-fea_delta", "d_a_t", "-d_win", "3", "-a_win", "1", "-t_win", "2"]


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def _chain(cfg):
    """(halo, largest window) of cfg's delta chain or stacking, from its own options."""
    opt = {k: v for k, v in zip(cfg[:-1], cfg[1:]) if k.startswith("-")}
    if "-fea_trap" in opt:
        w = (int(opt["-fea_trap"]) - 1) // 2
        return w, w
    if "-fea_delta" not in opt:
        return 0, 0
    ws = [int(opt.get(k, 2)) for k in ("-d_win", "-a_win", "-t_win")][:len(opt["-fea_delta"].split("_"))]
    return sum(ws), max(ws)


def _stream(eng, st, sid, x, chunks, cfg):
    """Pushes x in `chunks` on stream sid and finishes; the rows, after checking every push's count, st.frames and st.pending against R(F)."""
    H, wmax = _chain(cfg)
    assert streams_config_check(cfg, row_state=True) == (ceng.CTU_OK, "", H)
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
    assert got[-1].shape[0] == pending and st.frames(sid) == 0 and st.pending(sid) == 0
    return np.concatenate(got)


def _eights(eng, x):
    w, s = eng.dims.window, eng.dims.wshift
    return [w + 7 * s] + [8 * s] * 11 + [x.size - (w + 95 * s)]


@pytest.mark.parametrize("cfg", [C2 + DA, C2_8K + DA + ["-fea_Z_exp", "500"], C2 + ["-w", "40"] + DA, C2 + ["-fea_Z_block", "100"]],
                         ids=["d_a", "8k_d_a_Zexp", "1024_d_a", "Zblock"])
def test_pushes_of_eight_hops_are_bit_identical_to_the_offline_run(Engine, cfg):
    eng = Engine(cfg)
    x = _signal(eng, 96)
    off = eng.extract([x])[0]
    assert off.shape[0] == 96
    st = eng.streams(2, eng.dims.window + 8 * eng.dims.wshift, row_state=True)
    got = _stream(eng, st, 1, x, _eights(eng, x), cfg)
    assert got.shape == off.shape and np.array_equal(got, off)


def test_a_window_of_three_is_bit_identical_in_block_0_and_e_and_close_elsewhere(Engine):
    """Largest |streamed - offline| / max(|offline|, 1) over the delta blocks, measured on gfx950: 0.0 (the same expression in the same
    order compiles to the same multiply-adds; nothing holds a compiler to that, so the oracle bound is what is asserted)."""
    cfg = C2 + DAT312 + ["-fea_E", "on"]
    eng = Engine(cfg)
    x = _signal(eng, 96)
    off = eng.extract([x])[0]
    st = eng.streams(1, eng.dims.window + 8 * eng.dims.wshift, row_state=True)
    got = _stream(eng, st, 0, x, _eights(eng, x), cfg)
    assert got.shape == off.shape == (96, 53)
    assert np.array_equal(got[:, :13], off[:, :13]) and np.array_equal(got[:, 52], off[:, 52])
    print("d_a_t 3/1/2 + E streamed vs offline, largest |difference| / max(|offline|, 1):", float((np.abs(got - off) / np.maximum(np.abs(off), 1.0)).max()))
    _assert_rows(got, off, cfg)


@pytest.mark.parametrize("cfg", [
    C2 + DA,
    C2 + DAT312 + ["-fea_E", "on"],
    C2 + ["-fea_delta", "d_a_t", "-d_win", "1", "-a_win", "1", "-t_win", "1"],
    C2 + ["-fea_trap", "3"],
    C2 + ["-fea_trap", "9", "-fea_E", "on"],
    C2 + ["-fea_Z_exp", "500"],
    C2 + ["-fea_Z_block", "100"],
    C2 + ["-fea_Z_block", "300", "-fea_delta", "d_a", "-fea_E", "on"],
    C2 + ["-fea_Z_exp", "1000", "-fea_delta", "d"],
    C3 + ["-fea_Z_exp", "300", "-fea_delta", "d_a"],
    C2 + ["-fb_definition", "40filters", "-fea_ncepcoefs", "39"] + DA,
], ids=["d_a", "d_a_t_312_E", "d_a_t_111", "trap3", "trap9_E", "Zexp", "Zblock", "Zblock_d_a_E", "Zexp_d", "plp_Zexp_d_a", "hires_d_a"])
def test_arbitrary_chunking_agrees_with_the_oracle(Engine, cfg):
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 96)
    st = eng.streams(1, max(w, 17 * s), row_state=True)
    got = _stream(eng, st, 0, x, _schedule(eng, x.size, 11), cfg)
    ref = Oracle(cfg).process(x)
    assert got.shape == ref.shape and np.isfinite(got).all()
    _assert_rows(got, ref, cfg)


@pytest.mark.parametrize("extra, frames", [(DA, 4), (DAT312, 5)], ids=["d_a_4", "d_a_t_312_5"])
def test_a_file_no_longer_than_the_halo_comes_out_with_finish(Engine, extra, frames):
    cfg = C2 + extra
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, frames)
    st = eng.streams(1, w + 8 * s, row_state=True)
    for piece in (x[:w], x[w:w + s], x[w + s:]):
        assert st.push({0: piece})[0].shape[0] == 0
    assert st.frames(0) == 0 and st.pending(0) == frames
    got = st.finish(0)
    ref = Oracle(cfg).process(x)
    assert got.shape == ref.shape and ref.shape[0] == frames
    _assert_rows(got, ref, cfg)


def test_a_file_of_window_plus_one_frames_is_refused_at_finish_and_the_stream_starts_over(Engine):
    cfg = C2 + DA
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    y = _signal(eng, 40)
    chunks = _schedule(eng, y.size, 5)
    fresh = _stream(eng, eng.streams(1, max(w, 17 * s), row_state=True), 0, y, chunks, cfg)
    st = eng.streams(1, max(w, 17 * s), row_state=True)
    assert st.push({0: _signal(eng, 3)})[0].shape[0] == 0 and st.pending(0) == 3   # wmax + 1 frames
    with pytest.raises(CtuError) as ei:
        st.finish(0)
    assert ei.value.code == ceng.CTU_ERR_INPUT and "fewer than window+2" in str(ei.value)
    assert st.frames(0) == 0 and st.pending(0) == 0
    assert np.array_equal(_stream(eng, st, 0, y, chunks, cfg), fresh)


def test_a_stream_s_rows_do_not_depend_on_the_other_streams_or_on_the_file_before(Engine):
    cfg = C2_8K + DA + ["-fea_Z_exp", "500"]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    a, b, c = _signal(eng, 70), synth_utt(8, w + 30 * s, fs=8000), synth_utt(9, w + 40 * s + 5, fs=8000)
    ca = _schedule(eng, a.size, 3)
    alone = _stream(eng, eng.streams(1, max(w, 17 * s), row_state=True), 0, a, ca, cfg)
    st = eng.streams(4, max(w, 17 * s), row_state=True)   # A = stream 2, B = 0, C = 3
    rng = np.random.default_rng(4)
    at = {0: 0, 3: 0}
    got = {0: [], 2: [], 3: []}
    pos = 0
    for step, n_a in enumerate(ca):
        p = {2: a[pos:pos + n_a]}
        pos += n_a
        if step % 2:
            n_c = int(rng.integers(0, 4 * s))
            p[3] = c[at[3]:at[3] + n_c]
            at[3] += p[3].size
        for k, r in st.push(p).items():
            got[k].append(r)
        piece = b[at[0]:at[0] + int(rng.integers(s, 3 * s))]
        got[0].append(st.push({0: piece})[0])
        at[0] += piece.size
        if step == 9:   # B's file ends while A and C are under way; B starts another
            got[0].append(st.finish(0))
            _assert_rows(np.concatenate(got[0]), Oracle(cfg).process(b[:at[0]]), cfg)
            b, at[0], got[0] = b[at[0]:], 0, []
    got[2].append(st.finish(2))
    assert np.array_equal(np.concatenate(got[2]), alone)
    got[3].append(st.finish(3))
    _assert_rows(np.concatenate(got[3]), Oracle(cfg).process(c[:at[3]]), cfg)
    # a second file on stream 2: the history and the means were reset
    assert np.array_equal(_stream(eng, st, 2, a, ca, cfg), alone)


def test_the_flag_on_a_stateless_chain_changes_nothing(Engine):
    eng = Engine(C2)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 40)
    chunks = _schedule(eng, x.size, 2)
    plain, at = [], 0
    st0 = eng.streams(1, max(w, 17 * s))
    for c in chunks:
        plain.append(st0.push({0: x[at:at + c]})[0])
        at += c
    st = eng.streams(1, max(w, 17 * s), row_state=True)
    assert np.array_equal(_stream(eng, st, 0, x, chunks, C2), np.concatenate(plain))


def test_rows_that_do_not_fit_are_refused_before_anything_changes(Engine):
    import ctypes
    cfg = C2 + DA
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 40)
    st = eng.streams(2, w + 8 * s, row_state=True)
    L = ceng.load_library()
    first = st.push({0: x[:w + 7 * s]})[0]
    assert first.shape[0] == 4 and st.pending(0) == 4

    def raw_push(piece, cap):
        ids = np.array([0], dtype=np.int32)
        ns = np.array([piece.size], dtype=np.int64)
        buf = np.ascontiguousarray(piece)
        ptrs = (ctypes.c_void_p * 1)(buf.ctypes.data)
        rows = np.zeros((64, eng.dims.row_floats), dtype=np.float32)
        cnt = np.zeros(1, dtype=np.int64)
        return L.ctu_streams_push_host(st._h, 1, ids.ctypes.data, ptrs, ns.ctypes.data, rows.ctypes.data, cap, cnt.ctypes.data)

    assert raw_push(x[w + 7 * s:w + 15 * s], 7) == ceng.CTU_ERR_INPUT   # 8 rows into room for 7
    assert "rows_capacity" in L.ctu_last_error(eng._h).decode()
    rows = np.zeros((3, eng.dims.row_floats), dtype=np.float32)
    cnt = ctypes.c_int64(-1)
    assert L.ctu_streams_finish_host(st._h, 0, rows.ctypes.data, 3, ctypes.byref(cnt)) == ceng.CTU_ERR_INPUT   # 4 held back, room for 3
    assert st.frames(0) == 4 and st.pending(0) == 4
    got, at = [first], w + 7 * s
    for c in [8 * s, 8 * s, 8 * s, x.size - (w + 31 * s)]:
        got.append(st.push({0: x[at:at + c]})[0])
        at += c
    got.append(st.finish(0))
    assert np.array_equal(np.concatenate(got), eng.extract([x])[0])


def test_a_set_collected_in_a_cycle_with_its_engine_is_destroyed_ahead_of_it(Engine):
    """A caught CtuError's traceback ties a set and its engine into a reference cycle, and the collector finalises a cycle's objects in
    any order.  ctu_streams_destroy reads its engine: destroyed behind it, it selected a device ordinal out of freed memory and left
    the runtime's error behind for the next call that asks."""
    import gc
    cfg = C2 + DA
    eng = Engine(cfg)
    st = eng.streams(1, 1600, row_state=True)
    knot = [eng, st]          # the engine first: the order the collector meets them in
    knot.append(knot)
    handle = st._h.value
    del eng, st, knot
    gc.collect()
    eng = Engine(cfg)
    assert handle not in eng._sets
    st = eng.streams(1, 1600, row_state=True)
    x = _signal(eng, 12)
    assert st.push({0: x[:1600]})[0].shape[0] == eng.num_frames(1600) - 4   # (no stale error: the push's launch checks pass)
    eng.close()               # by hand in the wrong order: the engine takes its sets along, the set's own close finds nothing to do
    st.close()
