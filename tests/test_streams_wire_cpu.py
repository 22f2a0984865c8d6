"""Wire input (include/ctu_engine.h: ctu_wire_layout, ctu_streams_push_wire*) without a GPU: the exports and the binding's types, the
pure ctu_wire_expand against the reference's own G.711 tables (tests/golden/ref_outputs.npz) and numpy's byteswap, the pure
ctu_wire_extent against a brute-force count of the elements a push names, how both answer bad arguments - and that the calls that say
what a stream set takes answer as they did: the wire calls add no flag.
"""
import ctypes

import numpy as np
import pytest

from ctucopy_amd import CtuError, Streams, streams_config_check_ex, streams_flags_for, wire_expand, wire_extent
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from tests.test_streams_flags_for_cpu import ACCEPTED
from tests.util import ref_outputs

WIRE_EXPORTS = ["ctu_streams_push_wire", "ctu_streams_push_wire_host", "ctu_streams_push_signal_wire", "ctu_streams_push_signal_wire_host",
                "ctu_wire_extent", "ctu_wire_expand"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


def test_the_six_exports_exist_and_the_binding_types_them():
    L = ceng.load_library()
    vp, i32, i64, wl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ceng.WireLayout)
    for name in WIRE_EXPORTS:
        assert name in ceng.EXPORTS and hasattr(L, name), name
    assert ceng.WireLayout._fields_ == [("format", i32), ("stride", i32)] and ctypes.sizeof(ceng.WireLayout) == 8
    assert ceng.WIRE_FORMATS == {"s16": 0, "s16_swapped": 1, "alaw": 2, "mulaw": 3}
    assert L.ctu_streams_push_wire.argtypes == [vp, i32, vp, vp, vp, vp, wl, vp, i64, vp, vp, vp]
    assert L.ctu_streams_push_wire_host.argtypes == [vp, i32, vp, vp, vp, vp, wl, vp, i64, vp, vp]
    assert L.ctu_streams_push_signal_wire.argtypes == [vp, i32, vp, vp, vp, vp, wl, vp, i64, vp, vp]
    assert L.ctu_streams_push_signal_wire_host.argtypes == [vp, i32, vp, vp, vp, vp, wl, vp, i64, vp]
    assert L.ctu_wire_extent.restype == i64 and L.ctu_wire_extent.argtypes == [wl, i32, vp, vp, ctypes.POINTER(i64)]
    assert L.ctu_wire_expand.restype == i64 and L.ctu_wire_expand.argtypes == [wl, vp, i64, i64, vp]
    for name in ("push_wire", "push_wire_device", "push_signal_wire", "push_signal_wire_device", "push_interleaved"):
        assert callable(getattr(Streams, name)), name


@pytest.mark.parametrize("fmt,table", [("alaw", "amulaw_a"), ("mulaw", "amulaw_mu")])
def test_expand_gives_the_references_table_for_all_256_codes(fmt, table):
    ref = ref_outputs()[table]
    codes = np.arange(256, dtype=np.uint8)
    assert np.array_equal(wire_expand(codes, 0, 256, fmt), ref)
    back = codes[::-1].copy()
    assert np.array_equal(wire_expand(back, 0, 256, fmt), ref[back])
    # stride 3 from an offset: codes 5, 8, 11, ...
    assert np.array_equal(wire_expand(codes, 5, 83, fmt, stride=3), ref[5:5 + 3 * 83:3])


def test_expand_swaps_as_numpy_does_and_leaves_native_samples_alone():
    rng = np.random.default_rng(16)
    x = np.concatenate([np.array([-32768, 32767, 0, -1, 1, 255, 256, -256, 0x1234, -0x1234], dtype=np.int16),
                        rng.integers(-32768, 32768, size=1000).astype(np.int16)])
    assert np.array_equal(wire_expand(x, 0, x.size, "s16"), x)
    assert np.array_equal(wire_expand(x, 0, x.size, "s16_swapped"), x.byteswap())
    assert np.array_equal(wire_expand(x.byteswap(), 0, x.size, "s16_swapped"), x)
    for fmt, want in (("s16", x), ("s16_swapped", x.byteswap())):   # stride 3 from an offset picks elements 7, 10, 13, ...
        assert np.array_equal(wire_expand(x, 7, 300, fmt, stride=3), want[7:7 + 900:3])
        assert wire_expand(x, 7, 0, fmt, stride=3).size == 0


def _brute_extent(off, ns, stride):
    named = [int(o) + k * stride for o, n in zip(off, ns) for k in range(int(n))]
    return (max(named) - min(named) + 1, min(named)) if named else (0, 0)


@pytest.mark.parametrize("stride", [1, 2, 7, 64])
def test_extent_is_the_span_of_the_elements_a_push_names(stride):
    rng = np.random.default_rng(100 + stride)
    for trial in range(40):
        n = int(rng.integers(1, 9))
        ns = rng.integers(0, 40, size=n).astype(np.int64)
        ns[rng.random(n) < 0.3] = 0
        off = rng.integers(0, 500, size=n).astype(np.int64)
        off[ns == 0] = rng.integers(0, 10 ** 6, size=int((ns == 0).sum()))   # a stream without samples is not looked at
        for fmt in ("s16", "alaw"):
            assert wire_extent(off, ns, fmt, stride) == _brute_extent(off, ns, stride), (trial, fmt)
    assert wire_extent([5, 900, 33], [0, 0, 0], "mulaw", stride) == (0, 0)
    assert wire_extent([], [], "s16", stride) == (0, 0)
    assert wire_extent([11], [1], "s16_swapped", stride) == (1, 11)


def test_bad_arguments_come_back_negative_from_both_pure_calls():
    L = ceng.load_library()
    x = np.arange(64, dtype=np.int16)
    for args in (dict(elem_off=-1, n_samples=4), dict(elem_off=0, n_samples=4, stride=0), dict(elem_off=0, n_samples=4, stride=-3),
                 dict(elem_off=0, n_samples=4, fmt=4), dict(elem_off=0, n_samples=4, fmt=-1), dict(elem_off=0, n_samples=-2)):
        with pytest.raises(CtuError) as ei:
            wire_expand(x, **args)
        assert ei.value.code == ceng.CTU_ERR_INPUT
    for args in (dict(elem_off=[3, -1], n_samples=[4, 4]), dict(elem_off=[3, 1], n_samples=[4, 4], stride=0),
                 dict(elem_off=[3, 1], n_samples=[4, 4], fmt=7), dict(elem_off=[3, 1], n_samples=[4, -4])):
        with pytest.raises(CtuError) as ei:
            wire_extent(**args)
        assert ei.value.code == ceng.CTU_ERR_INPUT
    # the C calls themselves: a NULL layout, and 16-bit elements at an odd address
    out = np.zeros(8, dtype=np.int16)
    assert L.ctu_wire_expand(None, x.ctypes.data, 0, 4, out.ctypes.data) == ceng.CTU_ERR_INPUT
    assert L.ctu_wire_extent(None, 0, None, None, None) == ceng.CTU_ERR_INPUT
    w = ceng.WireLayout(0, 1)
    assert L.ctu_wire_expand(ctypes.byref(w), x.ctypes.data + 1, 0, 4, out.ctypes.data) == ceng.CTU_ERR_INPUT
    w = ceng.WireLayout(2, 1)   # codes lie at any address
    assert L.ctu_wire_expand(ctypes.byref(w), x.ctypes.data + 1, 0, 4, out.ctypes.data) == 4
    assert np.array_equal(out[:4], ref_outputs()["amulaw_a"][x.view(np.uint8)[1:5]])


def test_what_a_set_takes_is_answered_as_before():
    by_name = {c[0]: c for c in ACCEPTED}
    for name, flags, halo in (("C1", 0, 0), ("C4", ceng.STREAMS_NR_STATE | ceng.STREAMS_VAD_STATE, 1),
                              ("energy VAD + d_a", ceng.STREAMS_VAD_STATE | ceng.STREAMS_ROW_STATE | ceng.STREAMS_VAD_ROW_STATE, 5)):
        cfg = by_name[name][1]
        assert by_name[name][2:] == (flags, halo)
        assert streams_flags_for(cfg) == (ceng.CTU_OK, flags, "", halo)
        assert streams_config_check_ex(cfg, flags) == (ceng.CTU_OK, "", halo)
