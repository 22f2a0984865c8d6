"""Stream sets with subtraction state on the GPU (Engine.streams(..., ss_state=True)): -nr_mode hwss | fwss | 2fwss with the Burg-cepstral
detector behind pushed samples.  A stream's file gives the rows a FRESH engine's extract([x]) gives for that file alone - zero noise
seed, detector rebuilt - with the noise estimate(s) per bin and the detector's record kept per stream between the pushes.

The offline rows always come from a fresh Engine(cfg) (or one after reset_chain): an engine keeps the vector its last file left behind
from run to run, so a reused engine gives other rows.

Bounds: bit identity where DESIGN.md section 4.10 (Subtraction state) derives it - pushes that end a multiple of eight frames into the
file run the same instantiation over the same eight-frame steps, the decisions are doubles computed on identical spectra, and the
state's floats and doubles pass through memory as they stand - elsewhere the project's own rules for these modes against the oracle
(tests/test_gpu_parity.py: _assert_rows in the exten class for hwss / fwss, the rule of test_spectral_subtraction_at_16khz for 2fwss)."""
import numpy as np
import pytest

from ctucopy_amd import CtuError
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle
from tests.test_gpu_parity import SS8, _assert_rows
from tests.test_streams import _schedule, _signal
from tests.test_streams_nr import _eights, _rows_held, _stream   # (_stream counts every push by _chain of tests/test_streams_rows.py)
from tests.util import C2, sig

pytestmark = pytest.mark.gpu

C2B = C2 + ["-vad", "burg"]
FWSS = ["-nr_mode", "fwss"]
CONFIGS = [SS8 + FWSS, SS8 + ["-nr_mode", "2fwss", "-nr_p", "0.9", "-nr_q", "0.95"], SS8 + ["-nr_mode", "hwss", "-fea_kind", "spec"], C2B + FWSS,
           C2B + FWSS + ["-fea_E", "on"], SS8 + FWSS + ["-fb_eqld", "on", "-fb_inld", "on", "-fea_kind", "lpc", "-fea_lporder", "12"],
           SS8 + ["-nr_mode", "2fwss", "-fea_delta", "d_a", "-fea_Z_exp", "0.95"]]
IDS = ["fwss_8k", "2fwss_8k_p_q", "hwss_spec_8k", "fwss_16k", "fwss_16k_E", "fwss_8k_plp", "2fwss_8k_d_a_Zexp"]


@pytest.fixture(scope="module")
def Engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ctucopy_amd import Engine as E, load_library
    load_library()  # fails loudly when the HIP extension is missing
    return E


def _set(eng, cfg, n, max_push):
    return eng.streams(n, max_push, row_state=_rows_held(cfg), ss_state=True)


def _offline(Engine, cfg, x):
    return Engine(cfg).extract([x])[0]   # a fresh engine: zero seed


def _ss_rule(g, ref, cfg):
    """The project's own rule for these modes against the oracle (tests/test_gpu_parity.py)."""
    assert g.shape == ref.shape and np.isfinite(g).all()
    if "2fwss" in cfg:
        e = (np.abs(g - ref) / np.maximum(np.abs(ref), 1.0)).max(axis=1)
        rn = np.abs(g - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1.0)
        out = (e > 1e-3) | (rn > 1e-4)
        assert out.sum() <= max(1, ref.shape[0] // 100) and e.max() <= 5e-2, (int(out.sum()), float(e.max()), " ".join(cfg))
    else:
        _assert_rows(g, ref, cfg + ["-nr_mode", "exten"])


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_pushes_of_eight_hops_are_bit_identical_to_the_offline_run(Engine, cfg):
    eng = Engine(cfg)
    assert ", SS" in eng.kernel_name()
    x = _signal(eng, 96)
    off = _offline(Engine, cfg, x)
    assert off.shape[0] == 96
    chunks = _eights(eng, x)
    assert chunks[:2] == [eng.dims.window + 7 * eng.dims.wshift, 8 * eng.dims.wshift] and len(chunks) == 13
    st = _set(eng, cfg, 2, eng.dims.window + 8 * eng.dims.wshift)
    got = _stream(eng, st, 1, x, chunks, cfg)   # (frames and pending of every push against streams_rows_step)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("cfg", [SS8 + FWSS, C2B + FWSS], ids=["fwss_8k", "fwss_16k"])
def test_two_tiles_in_one_push_keep_the_state_in_registers_across_the_tile_edge(Engine, cfg):
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 96)
    off = _offline(Engine, cfg, x)
    chunks = _eights(eng, x, first=72)   # tiles of 64 and 8 frames, then three pushes that load the state from memory
    assert chunks[:4] == [w + 71 * s, 8 * s, 8 * s, 8 * s] and len(chunks) == 5
    st = _set(eng, cfg, 1, w + 71 * s)
    got = _stream(eng, st, 0, x, chunks, cfg)
    assert got.shape == off.shape and np.array_equal(got, off)


@pytest.mark.parametrize("cfg", [SS8 + FWSS, SS8 + ["-nr_mode", "hwss", "-fea_kind", "spec"], SS8 + ["-nr_mode", "2fwss"], C2B + FWSS, C2B + ["-nr_mode", "2fwss"]],
                         ids=["fwss_8k", "hwss_spec_8k", "2fwss_8k", "fwss_16k", "2fwss_16k"])
def test_arbitrary_chunking_agrees_with_the_oracle(Engine, cfg):
    """Largest |streamed - offline| / max(|offline|, 1) measured on gfx950 is in DESIGN.md section 4.10 (Subtraction state).  A flipped
    decision would show as a gross error from that frame on."""
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    x = _signal(eng, 96)
    st = _set(eng, cfg, 1, max(w, 17 * s))
    got = _stream(eng, st, 0, x, _schedule(eng, x.size, 11), cfg)
    ref = Oracle(cfg).process(x)
    off = _offline(Engine, cfg, x)
    assert got.shape == ref.shape == off.shape and np.isfinite(got).all()
    print("*ss streamed vs offline rows, largest |difference| / max(|offline|, 1):", float((np.abs(got - off) / np.maximum(np.abs(off), 1.0)).max()), " ".join(cfg))
    print("  element-wise error against the oracle: streamed", float((np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)).max()),
          "offline", float((np.abs(off - ref) / np.maximum(np.abs(ref), 1.0)).max()))
    _ss_rule(off, ref, cfg)   # an input that does not suit the rule shows on the offline side
    _ss_rule(got, ref, cfg)


def test_more_streams_than_chain_slots_hand_the_state_over_inside_one_chain(Engine):
    """A wave writes one stream's state out and reads the next stream's in inside one launch."""
    import torch
    cfg = SS8 + FWSS
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    n = 8 * 2 * torch.cuda.get_device_properties(0).multi_processor_count + 37   # 37 more than the chip holds waves of the front end
    sigs = [_signal(eng, 96, seed=40 + k) for k in range(4)]
    assert len({x.tobytes() for x in sigs}) == 4
    off = [_offline(Engine, cfg, x)[:24] for x in sigs]
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
    cfg = C2B + FWSS
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    n = _signal(eng, 40).size
    xa, xb, xc, xd1, xd2 = (sig("CS0")[k * 9001:k * 9001 + n].copy() for k in range(5))   # five stretches of the bundled recording
    offl = {name: _offline(Engine, cfg, x) for name, x in zip("abcd", (xa, xb, xc, xd2))}   # each from a fresh engine
    A, B, C, D = 3, 0, 2, 1
    alone_a = _stream(eng, _set(eng, cfg, 1, w + 8 * s), 0, xa, _eights(eng, xa), cfg)
    fresh_d = _stream(eng, _set(eng, cfg, 1, w + 8 * s), 0, xd2, _eights(eng, xd2), cfg)
    st = _set(eng, cfg, 4, w + 8 * s)
    got = {A: [], B: [], C: [], D: []}
    # ahead of the push in question: B and C have had a first push, D a whole file
    first = st.push({B: xb[:w + 7 * s], C: xc[:w + 7 * s]})
    got[B].append(first[B])
    got[C].append(first[C])
    assert np.array_equal(_stream(eng, st, D, xd1, _eights(eng, xd1), cfg), _offline(Engine, cfg, xd1))
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
    for k, name in ((A, "a"), (B, "b"), (C, "c"), (D, "d")):   # (C's pushes of eight hops still end eight frames apart: its half hop completes none)
        assert st.frames(k) == 40
        assert np.array_equal(np.concatenate(got[k]), offl[name]), name
    assert np.array_equal(np.concatenate(got[A]), alone_a)
    assert np.array_equal(np.concatenate(got[D]), fresh_d)   # the zero state was restored: the second file is a fresh engine's
    assert np.array_equal(fresh_d, offl["d"])


def test_the_engine_s_offline_chain_is_untouched_by_a_set(Engine):
    cfg = SS8 + FWSS
    a, b, x = (_signal(Engine(cfg), 60, seed=90 + k) for k in range(3))
    plain = Engine(cfg)
    want = [plain.extract([a])[0], plain.extract([b])[0]]
    assert not np.array_equal(want[1], _offline(Engine, cfg, b))   # the chain is real: b behind a is not b alone
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    first = eng.extract([a])[0]
    st = _set(eng, cfg, 2, w + 8 * s)
    got = _stream(eng, st, 0, x, _eights(eng, x), cfg)
    assert np.array_equal(got, _offline(Engine, cfg, x))             # the push read nothing of the offline chain
    second = eng.extract([b])[0]
    assert np.array_equal(first, want[0]) and np.array_equal(second, want[1])   # ... and wrote nothing of it


def test_without_the_flag_the_modes_have_no_stream_set(Engine):
    eng = Engine(SS8 + FWSS)
    for kw in ({}, {"row_state": True}, {"nr_state": True}):
        with pytest.raises(CtuError) as ei:
            eng.streams(2, 1600, **kw)
        assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED
        assert str(ei.value) == "ENGINE: configuration cannot be streamed: -nr_mode fwss (the noise estimate runs from frame to frame of a file)"
