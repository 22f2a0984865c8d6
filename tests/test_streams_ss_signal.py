"""Stream sets with subtraction state and signal state on the GPU (Engine.streams(..., signal_state=True, ss_state=True,
ss_signal_state=True)): the speech output of -nr_mode hwss | fwss | 2fwss with the Burg-cepstral detector behind pushed samples.  A
stream's file gives the samples a FRESH engine's enhance([x]) gives for that file alone - zero noise seed, detector rebuilt, tail zero -
with the noise estimate(s), the detector's record and the overlap-add's tail kept per stream between the pushes.

The offline samples always come from a fresh Engine(cfg): an engine keeps the vector its last file left behind from run to run.

Bounds.  Bit identity where DESIGN.md section 4.10 (Subtraction state with signal state) derives it: pushes that end a multiple of eight
frames into the file run the offline instantiation, up to the state traffic, over the same eight-frame steps of the same samples; the
state's floats and doubles pass through memory as they stand; and a sample's carried double partial sum continues the offline run's
additions in frame order.  Elsewhere the project's bound for this path against the oracle
(tests/test_gpu_parity.py::test_spectral_subtraction_with_signal_output): at most 2 LSB, mean at most 0.3 LSB - a flipped decision would
break it from that frame on.  Streamed against offline under other chunkings is measured and printed, not bounded in advance.

Inputs: tests/test_streams_ss_signal_cpu.py holds them (CASES) and checks on the oracle that each makes the detector take both decisions."""
import numpy as np
import pytest

from ctucopy_amd import CtuError
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_streams import _schedule
from tests.test_streams_signal import _lsb, _stream   # (_stream checks every push's count, frames and pending against ctu_streams_signal_step)
from tests.test_streams_ss_signal_cpu import CASES, case_input
from tests.util import ref_e2e, ref_e2e_inputs, REF_E2E_CASES, sig

pytestmark = pytest.mark.gpu

MAX_LSB, MEAN_LSB = 2, 0.3   # test_spectral_subtraction_with_signal_output's


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def _set(eng, n, max_push):
    return eng.streams(n, max_push, signal_state=True, ss_state=True, ss_signal_state=True)


def _offline(Engine, cfg, x):
    return Engine(cfg).enhance([x])[0]   # a fresh engine: zero seed


_cache = {}


def _case(Engine, name):
    """(configuration, 96 frames of input, a fresh engine's samples, the oracle's) of a case, made once for the module and left unchanged."""
    if name not in _cache:
        cfg, x = case_input(name)
        off, ref = _offline(Engine, cfg, x), Oracle(cfg).enhance(x)
        for a in (x, off, ref):
            a.setflags(write=False)
        _cache[name] = (cfg, x, off, ref)
    return _cache[name]


def _eights(eng, x, first=8):
    """A push that completes `first` frames, pushes of eight hops, the rest."""
    w, s = eng.dims.window, eng.dims.wshift
    out = [w + (first - 1) * s]
    while sum(out) + 8 * s <= x.size:
        out.append(8 * s)
    return out + [x.size - sum(out)]


def _oracle_bound(g, ref, what):
    d = _lsb(g, ref)
    assert g.shape == ref.shape and g.dtype == np.int16, (what, g.shape, ref.shape)
    assert d.max() <= MAX_LSB and d.mean() <= MEAN_LSB, (what, int(d.max()), float(d.mean()))


@pytest.mark.parametrize("name", ["fwss_16k", "fwss_8k", "2fwss_8k", "hwss_16k", "fwss_8k_a2_ncep5"])
def test_pushes_of_eight_hops_are_the_offline_samples_bit_for_bit(Engine, name):
    cfg, x, off, _ = _case(Engine, name)
    eng = Engine(cfg)
    assert eng.dims.signal_out == 1 and eng.kernel_name().endswith("SS, SY>")
    w, s = eng.dims.window, eng.dims.wshift
    assert off.size == 96 * s + w - s
    chunks = _eights(eng, x)
    assert chunks[:2] == [w + 7 * s, 8 * s] and len(chunks) == 13
    st = _set(eng, 2, w + 8 * s)
    got = _stream(eng, st, 1, x, chunks)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("name", ["fwss_16k", "fwss_8k"])
def test_a_first_push_of_two_tiles_keeps_the_state_in_registers_across_the_tile_edge(Engine, name):
    cfg, x, off, _ = _case(Engine, name)
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    chunks = _eights(eng, x, first=72)   # tiles of 64 and 8 frames - the tail written once from both - then pushes that load the state from memory
    assert chunks[:4] == [w + 71 * s, 8 * s, 8 * s, 8 * s] and len(chunks) == 5
    got = _stream(eng, _set(eng, 1, w + 71 * s), 0, x, chunks)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("name", ["fwss_16k", "fwss_8k", "2fwss_8k", "hwss_8k"])
def test_any_chunking_is_within_the_paths_bound_of_the_oracle(Engine, name):
    """Share of samples that differ from the offline run, and the worst difference, measured on gfx950: DESIGN.md section 4.10
    (Subtraction state with signal state)."""
    cfg, x, off, ref = _case(Engine, name)
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    _oracle_bound(off, ref, name + " offline")   # an input that does not suit the bound shows on the offline side
    chunks = _schedule(eng, x.size, 11)
    assert {0, 1, s - 1, w - 1, 7 * s, 9 * s, 17 * s} <= set(chunks)
    got = _stream(eng, _set(eng, 1, max(w, 17 * s)), 0, x, chunks)
    assert got.size == off.size
    d, do = _lsb(got, off), _lsb(got, ref)
    print("ss signal set %s: %.4f %% of the samples differ from the offline run, worst %d LSB; against the oracle max %d LSB, mean %.4f (offline: max %d, mean %.4f)"
          % (name, 100.0 * float((d > 0).mean()), int(d.max()), int(do.max()), float(do.mean()), int(_lsb(off, ref).max()), float(_lsb(off, ref).mean())))
    _oracle_bound(got, ref, name + " streamed")


def test_the_compiled_reference_s_first_file_in_pushes_of_nine_frames(Engine):
    """The first file of case sig_fwss (tests/golden/ref_e2e.npz) is a one-file process's output.  The rule of
    tests/test_ref_e2e_gpu.py::_assert_samples: within 2 LSB, mean below 0.3 LSB, at the rails within 2."""
    cfg, inp = REF_E2E_CASES["sig_fwss"]
    x = ref_e2e_inputs(inp)[0]
    ref = ref_e2e()["sig_fwss__0__pcm"]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    chunks = [w + 8 * s]
    while sum(chunks) + 9 * s <= x.size:
        chunks.append(9 * s)
    chunks.append(x.size - sum(chunks))
    got = _stream(eng, _set(eng, 1, w + 8 * s), 0, x, chunks)
    assert got.shape == ref.shape and got.dtype == np.int16, (got.shape, ref.shape)
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    rail = np.abs(ref.astype(np.int64)) >= 32767     # where the reference's overlap-add saturated
    at_rail = int(d[rail].max()) if rail.any() else 0
    print(f"sig_fwss[0] streamed in nines: max {int(d.max())} LSB, mean {d.mean():.4f} LSB, {int(rail.sum())} samples at a rail (max there {at_rail} LSB)")
    assert d.max() <= 2 and d.mean() < 0.3 and at_rail <= 2, (int(d.max()), float(d.mean()), at_rail)


def test_one_frame_per_push_carries_the_tail_over_itself(Engine):
    """-w 25 -s 10: (F1 - F0) * wshift = 160 < window - wshift = 240, so a new tail entry reads an old one further on, which the same
    launch replaces."""
    name = "fwss_16k_s10"
    cfg, x, off, ref = _case(Engine, name)
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    assert (w, s) == (400, 160) and off.size == 96 * s + w - s
    # pushes that land on multiples of eight frames: the offline samples
    got8 = _stream(eng, _set(eng, 1, w + 8 * s), 0, x, _eights(eng, x))
    assert np.array_equal(got8, off)
    # one frame per push: the oracle bound
    chunks = [w] + [s] * 95 + [x.size - w - 95 * s]
    st = _set(eng, 2, w)
    got = _stream(eng, st, 1, x, chunks)    # (its finish_signal delivers what pending says: the last window - wshift samples)
    d = _lsb(got, off)
    print("ss signal set, one frame per push: %.4f %% of the samples differ from the offline run, worst %d LSB" % (100.0 * float((d > 0).mean()), int(d.max())))
    assert got.size == off.size
    _oracle_bound(off, ref, name + " offline")
    _oracle_bound(got, ref, name + " one frame per push")
    # the tail alone: 96 one-frame pushes again, then the finish
    at = 0
    for c in chunks:
        st.push_signal({0: x[at:at + c]})
        at += c
    assert st.pending(0) == 240
    tail = st.finish_signal(0)
    assert tail.size == 240 and np.array_equal(tail, got[-240:])


def test_more_streams_than_chain_slots_hand_the_state_over_inside_one_chain(Engine):
    """A wave stores one stream's slot and loads the next stream's inside one launch, and every stream has its own tail."""
    import torch
    cfg = CASES["fwss_16k"][0]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    n = 8 * 2 * torch.cuda.get_device_properties(0).multi_processor_count + 37   # 37 more than the chip holds waves of the front end
    size = w + 23 * s + s // 2
    sigs = [sig("CS0")[k * 9001:k * 9001 + size].copy() for k in range(4)]
    assert len({x.tobytes() for x in sigs}) == 4
    off = [_offline(Engine, cfg, x)[:24 * s] for x in sigs]   # (frame t reaches no sample ahead of t s: the first 24 s samples are complete)
    st = _set(eng, n, w + 7 * s)
    got, at = [[] for _ in range(n)], 0
    for c in (w + 7 * s, 8 * s, 8 * s):
        out = st.push_signal({i: sigs[i % 4][at:at + c] for i in range(n)})
        at += c
        for i in range(n):
            assert out[i].size == 8 * s
            got[i].append(out[i].copy())
    wrong = [i for i in range(n) if not np.array_equal(np.concatenate(got[i]), off[i % 4])]
    assert not wrong, (len(wrong), wrong[:8])


def test_streams_in_different_phases_share_a_push(Engine):
    cfg = CASES["fwss_16k"][0]
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    n = w + 39 * s + s // 2
    xa, xb, xc, xd1, xd2 = (sig("CS0")[k * 9001:k * 9001 + n].copy() for k in range(5))   # five stretches of the bundled recording
    sigs = {3: xa, 0: xb, 2: xc, 1: xd2}
    A, B, C, D = 3, 0, 2, 1
    rest = lambda x, first: first + [8 * s] * ((x.size - sum(first)) // (8 * s)) + [(x.size - sum(first)) % (8 * s)]
    plan = {A: rest(xa, [w + 7 * s]), B: rest(xb, [w + 7 * s, 8 * s]), C: rest(xc, [w + 7 * s, s // 2]), D: rest(xd2, [w + 7 * s])}
    assert all(sum(plan[k]) == sigs[k].size for k in plan)
    st = _set(eng, 4, w + 8 * s)
    got = {k: [] for k in plan}
    # ahead of the push in question: B and C have had a first push, D a whole file
    first = st.push_signal({B: xb[:plan[B][0]], C: xc[:plan[C][0]]})
    at = {A: 0, B: plan[B][0], C: plan[C][0], D: 0}
    step = {A: 0, B: 1, C: 1, D: 0}
    got[B].append(first[B].copy())
    got[C].append(first[C].copy())
    assert np.array_equal(_stream(eng, st, D, xd1, _eights(eng, xd1)), _offline(Engine, cfg, xd1))
    # the push: A starts a file, B goes on, C completes no frame, D starts its second file
    out = st.push_signal({k: sigs[k][at[k]:at[k] + plan[k][step[k]]] for k in (A, B, C, D)})
    assert [out[k].size for k in (A, B, C, D)] == [8 * s, 8 * s, 0, 8 * s]
    for k in (A, B, C, D):
        got[k].append(out[k].copy())
        at[k] += plan[k][step[k]]
        step[k] += 1
    while any(step[k] < len(plan[k]) for k in plan):
        p = {k: sigs[k][at[k]:at[k] + plan[k][step[k]]] for k in plan if step[k] < len(plan[k])}
        for k, r in st.push_signal(p).items():
            got[k].append(r.copy())
            at[k] += p[k].size
            step[k] += 1
    for k in plan:
        assert st.frames(k) == 40
        got[k].append(st.finish_signal(k).copy())
        alone = _stream(eng, _set(eng, 1, w + 8 * s), 0, sigs[k], plan[k])
        assert np.array_equal(np.concatenate(got[k]), alone), k
        # every stream's pushes end a multiple of eight frames into its file (C's half hop completes none): a fresh engine's samples,
        # and D's second file starts clean - zero seed, detector rebuilt, tail zero
        assert np.array_equal(np.concatenate(got[k]), _offline(Engine, cfg, sigs[k])), k


def test_the_engine_s_offline_chain_is_untouched_by_a_set(Engine):
    cfg = CASES["fwss_8k"][0]
    a, b, x = (case_input("fwss_8k", 60)[1], case_input("2fwss_8k", 60)[1][::-1].copy(), _case(Engine, "fwss_8k")[1])
    plain = Engine(cfg)
    want = [plain.enhance([a])[0], plain.enhance([b])[0]]
    assert not np.array_equal(want[1], _offline(Engine, cfg, b))   # the chain is real: b behind a is not b alone
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    first = eng.enhance([a])[0]
    got = _stream(eng, _set(eng, 2, w + 8 * s), 0, x, _eights(eng, x))
    assert np.array_equal(got, _case(Engine, "fwss_8k")[2])          # the pushes read nothing of the offline chain
    second = eng.enhance([b])[0]
    assert np.array_equal(first, want[0]) and np.array_equal(second, want[1])   # ... and wrote nothing of it


def test_wrong_calls_and_flags_are_refused_before_anything_changes(Engine):
    cfg, x, off, _ = _case(Engine, "fwss_16k")
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    st = _set(eng, 2, w + 8 * s)
    assert np.array_equal(st.push_signal({0: x[:w + 7 * s]})[0], off[:8 * s])
    with pytest.raises(CtuError) as ei:
        st.push({0: x[:s]})
    assert ei.value.code == ceng.CTU_ERR_INPUT and "ctu_streams_push_signal / ctu_streams_finish_signal" in str(ei.value)
    assert st.frames(0) == 8 and st.pending(0) == w - s
    assert np.array_equal(st.push_signal({0: x[w + 7 * s:w + 15 * s]})[0], off[8 * s:16 * s])
    with pytest.raises(CtuError) as ei:
        st.finish(0)
    assert ei.value.code == ceng.CTU_ERR_INPUT and "ctu_streams_push_signal / ctu_streams_finish_signal" in str(ei.value)
    assert st.frames(0) == 16 and st.pending(0) == w - s
    assert np.array_equal(st.push_signal({0: x[w + 15 * s:w + 23 * s]})[0], off[16 * s:24 * s])
    # the two states without the flag that joins them: today's sentence
    for kw in ({"ss_state": True, "signal_state": True}, {"ss_state": True, "signal_state": True, "row_state": True, "nr_state": True}):
        with pytest.raises(CtuError) as ei:
            eng.streams(2, w + 8 * s, **kw)
        assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED
        assert str(ei.value) == ("ENGINE: configuration cannot be streamed: -nr_mode fwss with -format_out raw | wave (speech output behind hwss / fwss / 2fwss "
                                 "is not streamed, whatever the signal flag: the subtraction state serves the feature path)")
    with pytest.raises(CtuError) as ei:
        eng.streams(2, w + 8 * s, ss_signal_state=True)
    assert ei.value.code == ceng.CTU_ERR_INPUT and str(ei.value) == "ENGINE: unknown stream set flags"
    assert np.array_equal(st.push_signal({0: x[w + 23 * s:w + 31 * s]})[0], off[24 * s:32 * s])
    # a file shorter than one frame on the other stream (the reference's words), which is reset all the same
    assert st.push_signal({1: x[:w - s - 1]})[1].size == 0
    with pytest.raises(CtuError, match="Signal shorter than one frame!") as ei:
        st.finish_signal(1)
    assert ei.value.code == ceng.CTU_ERR_INPUT and st.frames(1) == 0 and st.pending(1) == 0
    assert np.array_equal(st.push_signal({0: x[w + 31 * s:w + 39 * s], 1: x[:w + 7 * s]})[1], off[:8 * s])
    assert st.frames(0) == 40 and st.frames(1) == 8
