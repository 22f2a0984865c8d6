"""Stream sets with subtraction state on large transforms on the GPU (Engine.streams(..., ss_state=True, ss_large_state=True)): -nr_mode
hwss | fwss | 2fwss with the Burg-cepstral detector on 2048- and 4096-point frames behind pushed samples.  A stream's file gives the rows a
FRESH engine's extract([x]) gives for that file alone - zero noise seed, detector rebuilt - with both noise estimates and the detector's
record kept per stream between the pushes (bigss_kernel<NIT, true>, ss_decide_stream_kernel).

The offline rows always come from a fresh Engine(cfg): an engine keeps the vector its last file left behind from run to run.

Bounds: bit identity for ANY chunking (Subtraction state on large transforms) - the export and the detector's
cepstra are per frame, the decisions and both estimates are doubles that pass through memory as they stand, a single file offline is
one pass from a zero seed, offline and streamed kernel share the frame's step (bigss_frame_step), and none of these kernels works in
steps of eight frames as the small front end does.  Against the oracle the rule of tests/test_ss_big.py (assert_rows), imported.
Signals are 40 to 48 frames at 1103 / 441 (2048 points) and 3072 / 960 samples (4096 points), but for the test of a push across a
tile edge, which needs more than a tile."""
import numpy as np
import pytest

from ctucopy_amd import CtuError, config_table
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_ss_big import assert_rows, the_list
from tests.test_ss_big_cpu import SIGNAL_CONFIGS
from tests.test_streams import _schedule
from tests.test_streams_nr import _rows_held, _stream   # (_stream counts every push by _chain of tests/test_streams_rows.py, and finishes)
from tests.test_streams_ss_large_cpu import CHAIN, TAKEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def _set(eng, cfg, n, max_push):
    return eng.streams(n, max_push, row_state=_rows_held(cfg), ss_state=True, ss_large_state=True)


_OFF = {}


def _offline(Engine, cfg, x):
    """A fresh engine's rows of x alone (zero seed); computed once per (configuration, signal) and shared, never written."""
    key = (" ".join(cfg), x.tobytes())
    if key not in _OFF:
        rows = Engine(cfg).extract([x])[0]
        rows.setflags(write=False)
        _OFF[key] = rows
    return _OFF[key]


def _sig(cfg, eng, frames, k=1, at=0):
    """`frames` frames and half a hop that completes none, out of file k of the list of tests/test_ss_big.py (its inputs suit the modes)."""
    n = eng.dims.window + (frames - 1) * eng.dims.wshift + eng.dims.wshift // 2
    x = the_list(cfg)[k][at:at + n].copy()
    assert x.size == n and eng.num_frames(n) == frames
    return x


def _kernel(cfg):
    return "bigss_kernel<16>" if "48000" in cfg else "bigss_kernel<8>"


@pytest.mark.parametrize("name", list(TAKEN))
def test_any_chunking_is_bit_identical_to_a_fresh_engines_rows(Engine, name):
    cfg = TAKEN[name]
    eng = Engine(cfg)
    assert eng.kernel_name() == _kernel(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    assert (w, s) == ((3072, 960) if "48000" in cfg else (1103, 441))
    x = _sig(cfg, eng, 44)
    off = _offline(Engine, cfg, x)
    assert off.shape[0] == 44 and np.isfinite(off).all()
    st = _set(eng, cfg, 2, max(w, 17 * s))
    hops = [w] + [s] * 43 + [x.size - (w + 43 * s)]   # pushes of exactly one hop: a frame each
    for tag, chunks in (("schedule 11", _schedule(eng, x.size, 11)), ("schedule 23", _schedule(eng, x.size, 23)), ("one hop", hops)):
        got = _stream(eng, st, 1, x, chunks, cfg)   # (every file of stream 1 is a first file: the finish inside _stream resets it)
        assert got.shape == off.shape
        print(f"{name}, {tag}: {len(chunks)} pushes, largest |streamed - offline| {float(np.abs(got - off).max()):.3g}")
        assert np.array_equal(got, off), (name, tag)


@pytest.mark.parametrize("name", ["fwss_44k", "fwss_48k_w64"])
def test_a_first_push_that_spans_two_tiles_then_pushes_that_load_the_state(Engine, name):
    cfg = TAKEN[name]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    tile = int(config_table(cfg, "tile_frames")[0])   # frames per tile record of the set's plan
    assert tile >= 8
    frames = tile + 8 + 9
    n = w + (frames - 1) * s + s // 2
    x = np.concatenate(the_list(cfg)[:4])[:n].copy()
    assert x.size == n
    off = _offline(Engine, cfg, x)
    assert off.shape[0] == frames
    chunks = [w + (tile + 7) * s, 3 * s, 3 * s, 3 * s, x.size - (w + (tile + 16) * s)]   # tiles of `tile` and 8 frames, then the state from memory
    st = _set(eng, cfg, 1, chunks[0])
    got = _stream(eng, st, 0, x, chunks, cfg)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("points", [2048, 4096])
def test_more_streams_than_chain_slots_hand_the_state_over_inside_one_chain(Engine, points):
    """A workgroup stores one stream's slot and loads the next stream's inside one launch.  -nr_initsegs 2: the decisions gate the
    update from the third frame on, so the detector's record matters in every push."""
    import torch
    cfg = TAKEN["fwss_44k" if points == 2048 else "fwss_48k_w64"] + ["-nr_initsegs", "2"]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 37   # 37 more than bigss_kernel's eight workgroup chains a CU
    sigs = [_sig(cfg, eng, 12, k=k % 3, at=5000 * (k // 3)) for k in range(4)]
    assert len({x.tobytes() for x in sigs}) == 4
    off = [_offline(Engine, cfg, x) for x in sigs]
    st = _set(eng, cfg, n, w + 3 * s)
    got, at = [[] for _ in range(n)], 0
    for c in (w + 3 * s, 4 * s, 4 * s):
        out = st.push({i: sigs[i % 4][at:at + c] for i in range(n)})
        at += c
        for i in range(n):
            assert out[i].shape[0] == 4
            got[i].append(out[i])
    wrong = [i for i in range(n) if not np.array_equal(np.concatenate(got[i]), off[i % 4])]
    assert not wrong, (len(wrong), wrong[:8])


@pytest.mark.parametrize("name", ["fwss_44k", "2fwss_44k_p_q"])
def test_streams_in_different_phases_share_a_push(Engine, name):
    cfg = TAKEN[name]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    xa, xb, xc, xd1, xd2 = (_sig(cfg, eng, 40, k=k % 3, at=4000 * (k // 3)) for k in range(5))
    assert len({v.tobytes() for v in (xa, xb, xc, xd1, xd2)}) == 5
    offl = {nm: _offline(Engine, cfg, x) for nm, x in zip("abcd", (xa, xb, xc, xd2))}   # each from a fresh engine
    A, B, C, D = 3, 0, 2, 1
    st = _set(eng, cfg, 4, w + 8 * s)
    got = {A: [], B: [], C: [], D: []}
    # ahead of the push in question: B and C have had a first push, D a whole file and its finish
    first = st.push({B: xb[:w + 4 * s], C: xc[:w + 4 * s]})
    got[B].append(first[B])
    got[C].append(first[C])
    fives = lambda x: [w + 4 * s] + [5 * s] * 7 + [x.size - (w + 39 * s)]
    assert np.array_equal(_stream(eng, st, D, xd1, fives(xd1), cfg), _offline(Engine, cfg, xd1))
    # the push: A starts a file, B goes on, C completes no frame, D starts its second file
    at = {A: 0, B: w + 4 * s, C: w + 4 * s, D: 0}
    sigs = {A: xa, B: xb, C: xc, D: xd2}
    step = {A: w + 4 * s, B: 5 * s, C: s // 2, D: w + 4 * s}
    out = st.push({k: sigs[k][at[k]:at[k] + step[k]] for k in (A, B, C, D)})
    assert [out[k].shape[0] for k in (A, B, C, D)] == [5, 5, 0, 5]
    for k in (A, B, C, D):
        got[k].append(out[k])
        at[k] += step[k]
    while any(at[k] < sigs[k].size for k in sigs):
        p = {k: sigs[k][at[k]:at[k] + 5 * s] for k in sigs if at[k] < sigs[k].size}
        for k, r in st.push(p).items():
            got[k].append(r)
            at[k] += p[k].size
    for k, nm in ((A, "a"), (B, "b"), (C, "c"), (D, "d")):   # (D: the second file alone, from a zero seed and a detector afresh)
        assert st.frames(k) == 40
        assert np.array_equal(np.concatenate(got[k]), offl[nm]), nm


def test_a_2fwss_delta_cms_chain_with_row_state(Engine):
    cfg = CHAIN
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _sig(cfg, eng, 48)
    off = _offline(Engine, cfg, x)
    assert off.shape[0] == 48
    st = _set(eng, cfg, 2, max(w, 17 * s))
    first = st.push({1: x[:w + 9 * s]})[1]
    assert first.shape[0] == 10 - 4 and st.pending(1) == 4   # rows leave with the chain's delay (halo 2 + 2)
    assert np.array_equal(first, off[:6])
    st.finish(1)
    got = _stream(eng, st, 1, x, _schedule(eng, x.size, 5), cfg)   # (finish delivers the rest: _stream checks the counts)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("name", ["fwss_44k", "hwss_spec_44k_a2_b15", "2fwss_44k_p_q", "fwss_48k_w64"])
def test_streamed_and_offline_rows_against_the_oracle(Engine, name):
    cfg = TAKEN[name]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    st = _set(eng, cfg, 1, max(w, 17 * s))
    for k, x in enumerate(the_list(cfg)[:2]):
        ref = Oracle(cfg).process(x)   # a fresh oracle per file: every file of a stream is a first file
        off = _offline(Engine, cfg, x)
        assert_rows(off, ref, cfg, f"{name} file {k} offline")   # an input that does not suit the rule shows on the offline side
        got = _stream(eng, st, 0, x, _schedule(eng, x.size, 11 + k), cfg)
        assert_rows(got, ref, cfg, f"{name} file {k} streamed")


def test_the_engines_offline_chain_is_untouched_by_a_set(Engine):
    cfg = TAKEN["fwss_44k"]
    probe = Engine(cfg)
    a, b, x = (_sig(cfg, probe, 40, k=k) for k in range(3))
    plain = Engine(cfg)
    want = [plain.extract([a])[0], plain.extract([b])[0]]
    assert not np.array_equal(want[1], _offline(Engine, cfg, b))   # the chain is real: b behind a is not b alone
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    first = eng.extract([a])[0]
    st = _set(eng, cfg, 2, max(w, 17 * s))
    got = _stream(eng, st, 0, x, _schedule(eng, x.size, 3), cfg)
    assert np.array_equal(got, _offline(Engine, cfg, x))             # the push read nothing of the offline chain
    second = eng.extract([b])[0]
    assert np.array_equal(first, want[0]) and np.array_equal(second, want[1])   # ... and wrote nothing of it


def test_without_the_flag_the_set_is_refused_and_speech_output_is_refused_by_name(Engine):
    cfg = TAKEN["fwss_44k"]
    eng = Engine(cfg)
    for kw, why in (({}, "-nr_mode fwss (the noise estimate runs from frame to frame of a file)"),
                    ({"ss_state": True}, "-nr_mode fwss on 2048-point frames (-w: the passes of the large transforms' subtraction are not streamed, "
                                         "a stream set carries the one of the 256- and 512-point front end)"),
                    ({"ss_state": True, "nr_state": True, "large_state": True}, "-nr_mode fwss on 2048-point frames (-w: the passes of the large transforms' "
                     "subtraction are not streamed, a stream set carries the one of the 256- and 512-point front end)")):
        with pytest.raises(CtuError) as ei:
            eng.streams(2, 4000, **kw)
        assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED and str(ei.value) == "ENGINE: configuration cannot be streamed: " + why
    with pytest.raises(CtuError) as ei:
        eng.streams(2, 4000, ss_large_state=True)
    assert ei.value.code == ceng.CTU_ERR_INPUT and str(ei.value) == "ENGINE: unknown stream set flags"
    for scfg, word in zip(SIGNAL_CONFIGS, ("-nr_mode fwss with -format_out raw | wave on 2048-point frames", "-nr_mode 2fwss with -format_out raw | wave on 4096-point frames")):
        with pytest.raises(CtuError) as ei:
            Engine(scfg).streams(2, 8000, True, True, True, True, True, True, True, True, True)   # every flag
        assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED
        assert str(ei.value).startswith("ENGINE: configuration cannot be streamed: " + word + " (speech output behind the large transforms' subtraction is not streamed"), str(ei.value)
