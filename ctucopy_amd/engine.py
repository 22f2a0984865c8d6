"""ctypes binding of include/ctu_engine.h -- the only way Python reaches the hot path.

PyTorch is used purely as plumbing (device buffers and streams); the computation is the HIP library.
There is no CPU fallback: creating an Engine without the built library or without a GPU raises.
"""
import ctypes
import os
import weakref

import numpy as np

from . import build as _build

CTU_OK, CTU_ERR_OPTS, CTU_ERR_UNSUPPORTED, CTU_ERR_DEVICE, CTU_ERR_INPUT = 0, -1, -2, -3, -4
STREAMS_ROW_STATE = 1  # CTU_STREAMS_ROW_STATE
STREAMS_NR_STATE = 4   # CTU_STREAMS_NR_STATE
STREAMS_VAD_STATE = 8  # CTU_STREAMS_VAD_STATE
STREAMS_SIGNAL_STATE = 32  # CTU_STREAMS_SIGNAL_STATE (2 and 16 are no flags)
STREAMS_LARGE_STATE = 64   # CTU_STREAMS_LARGE_STATE
STREAMS_TRAP_STATE = 256   # CTU_STREAMS_TRAP_STATE (128 is no flag either)
STREAMS_SS_STATE = 1024    # CTU_STREAMS_SS_STATE (nor is 512)
STREAMS_SS_SIGNAL_STATE = 2048  # CTU_STREAMS_SS_SIGNAL_STATE (a flag beside STREAMS_SS_STATE and STREAMS_SIGNAL_STATE only)
STREAMS_SS_LARGE_STATE = 8192   # CTU_STREAMS_SS_LARGE_STATE (a flag beside STREAMS_SS_STATE only; 4096 is no flag)
STREAMS_VAD_ROW_STATE = 16384   # CTU_STREAMS_VAD_ROW_STATE (a flag beside STREAMS_ROW_STATE and STREAMS_VAD_STATE only)


class CtuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


WIRE_FORMATS = {"s16": 0, "s16_swapped": 1, "alaw": 2, "mulaw": 3}  # CTU_WIRE_*


class WireLayout(ctypes.Structure):
    """ctu_wire_layout: how a stream's new samples lie in a buffer."""
    _fields_ = [("format", ctypes.c_int32), ("stride", ctypes.c_int32)]


class Dims(ctypes.Structure):
    _fields_ = [("fs", ctypes.c_int32), ("window", ctypes.c_int32), ("wshift", ctypes.c_int32),
                ("wfft", ctypes.c_int32), ("nbins", ctypes.c_int32), ("nbands", ctypes.c_int32),
                ("row_floats", ctypes.c_int32), ("htk_kind", ctypes.c_int32), ("htk_period", ctypes.c_uint32),
                ("has_vad", ctypes.c_int32), ("swap_out", ctypes.c_int32), ("pcm_align", ctypes.c_int32),
                ("signal_out", ctypes.c_int32), ("rows_in", ctypes.c_int32), ("row_floats_in", ctypes.c_int32),
                ("swap_in", ctypes.c_int32)]


# every symbol include/ctu_engine.h declares (checked by tests/test_abi.py)
EXPORTS = ["ctu_engine_create", "ctu_engine_destroy", "ctu_create_error", "ctu_last_error", "ctu_engine_dims",
           "ctu_config_dims", "ctu_config_table", "ctu_num_frames", "ctu_plan_create", "ctu_plan_destroy", "ctu_plan_sample_offsets",
           "ctu_plan_row_offsets", "ctu_arena_layout", "ctu_plan_total_samples", "ctu_plan_total_frames", "ctu_engine_run",
           "ctu_engine_run_host", "ctu_host_alloc", "ctu_host_free", "ctu_engine_reset_chain", "ctu_engine_set_vad_stream", "ctu_vad_ring_step", "ctu_plan_set_vad_ring", "ctu_vad_ring_rows", "ctu_decode_g711", "ctu_engine_last_kernel_ms", "ctu_engine_kernel_name", "ctu_engine_phase2_walk", "ctu_cmvn_cols", "ctu_cmvn_accumulate", "ctu_cmvn_apply",
           "ctu_cmvn_accumulate_host", "ctu_cmvn_apply_host", "ctu_plan_out_samples", "ctu_engine_run_signal",
           "ctu_engine_run_signal_host", "ctu_rows_arena_layout", "ctu_engine_run_rows", "ctu_engine_run_rows_host",
           "ctu_streams_create", "ctu_streams_destroy", "ctu_streams_config_check", "ctu_streams_push", "ctu_streams_push_host",
           "ctu_streams_finish", "ctu_streams_frames", "ctu_streams_step", "ctu_streams_last_push_ms",
           "ctu_streams_create_ex", "ctu_streams_config_check_ex", "ctu_streams_pending", "ctu_streams_finish_host", "ctu_streams_rows_step",
           "ctu_streams_push_vad", "ctu_streams_push_vad_host", "ctu_streams_finish_vad", "ctu_streams_finish_vad_host", "ctu_streams_vad_step",
           "ctu_streams_push_signal", "ctu_streams_push_signal_host", "ctu_streams_finish_signal", "ctu_streams_finish_signal_host", "ctu_streams_signal_step",
           "ctu_streams_vad_rows_step", "ctu_streams_flags_for",
           "ctu_streams_push_wire", "ctu_streams_push_wire_host", "ctu_streams_push_signal_wire", "ctu_streams_push_signal_wire_host",
           "ctu_wire_extent", "ctu_wire_expand",
           "ctu_plan_unpack_wire", "ctu_engine_run_wire_host", "ctu_engine_run_signal_wire_host"]

_lib = None


def load_library():
    """Loads ctucopy_amd/libctu_engine.so (must have been built: __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("CTU_ENGINE_LIB", _build.LIB)  # override only for A/B experiments on kernel builds
    if not os.path.exists(path):
        raise CtuError(CTU_ERR_DEVICE, f"{path} is missing: run __graft_entry__.build() (hipcc, gfx950) first; "
                                       "there is no CPU fallback")
    L = ctypes.CDLL(path)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    argv_t = ctypes.POINTER(ctypes.c_char_p)
    L.ctu_engine_create.argtypes = [ctypes.c_int, argv_t, ctypes.c_int, ctypes.POINTER(vp)]
    L.ctu_engine_destroy.argtypes = [vp]
    L.ctu_create_error.restype = ctypes.c_char_p
    L.ctu_last_error.restype = ctypes.c_char_p
    L.ctu_last_error.argtypes = [vp]
    L.ctu_engine_dims.argtypes = [vp, ctypes.POINTER(Dims)]
    L.ctu_config_dims.argtypes = [ctypes.c_int, argv_t, ctypes.POINTER(Dims)]
    L.ctu_config_table.restype = i64
    L.ctu_config_table.argtypes = [ctypes.c_int, argv_t, ctypes.c_char_p, vp, i64]
    L.ctu_num_frames.restype = i64
    L.ctu_num_frames.argtypes = [vp, i64]
    L.ctu_plan_create.argtypes = [vp, ctypes.POINTER(i64), i32, ctypes.POINTER(vp)]
    L.ctu_plan_destroy.argtypes = [vp]
    L.ctu_plan_sample_offsets.restype = ctypes.POINTER(i64)
    L.ctu_plan_sample_offsets.argtypes = [vp]
    L.ctu_plan_row_offsets.restype = ctypes.POINTER(i64)
    L.ctu_plan_row_offsets.argtypes = [vp]
    L.ctu_arena_layout.restype = i64
    L.ctu_arena_layout.argtypes = [ctypes.POINTER(i64), ctypes.c_int32, ctypes.POINTER(i64)]
    L.ctu_plan_total_samples.restype = i64
    L.ctu_plan_total_samples.argtypes = [vp]
    L.ctu_plan_total_frames.restype = i64
    L.ctu_plan_total_frames.argtypes = [vp]
    L.ctu_engine_run.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ctu_engine_run_host.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ctu_engine_reset_chain.argtypes = [vp]
    L.ctu_engine_set_vad_stream.argtypes = [vp, ctypes.c_char_p, i64]
    L.ctu_vad_ring_step.restype = None
    L.ctu_vad_ring_step.argtypes = [ctypes.c_int32, i64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.ctu_plan_set_vad_ring.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.ctu_vad_ring_rows.restype = i64
    L.ctu_vad_ring_rows.argtypes = [ctypes.c_int32, i64, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    L.ctu_decode_g711.argtypes = [vp, vp, i64, ctypes.c_int, vp, vp]
    L.ctu_host_alloc.restype = vp
    L.ctu_host_alloc.argtypes = [ctypes.c_size_t]
    L.ctu_host_free.argtypes = [vp]
    L.ctu_engine_last_kernel_ms.restype = ctypes.c_float
    L.ctu_engine_last_kernel_ms.argtypes = [vp]
    L.ctu_engine_kernel_name.restype = ctypes.c_char_p
    L.ctu_engine_kernel_name.argtypes = [vp]
    if hasattr(L, "ctu_engine_phase2_walk"):  # absent from older builds loaded through CTU_ENGINE_LIB for an A/B
        L.ctu_engine_phase2_walk.argtypes = [vp]
    L.ctu_cmvn_cols.argtypes = [vp]
    L.ctu_cmvn_accumulate.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.ctu_cmvn_apply.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.ctu_cmvn_accumulate_host.argtypes = [vp, vp, vp, vp, i32, vp, vp]
    L.ctu_plan_out_samples.restype = ctypes.POINTER(i64)
    L.ctu_plan_out_samples.argtypes = [vp]
    L.ctu_engine_run_signal.argtypes = [vp, vp, vp, vp, vp]
    L.ctu_engine_run_signal_host.argtypes = [vp, vp, vp, vp]
    L.ctu_cmvn_apply_host.argtypes = [vp, vp, vp, vp, i32, vp, vp]
    L.ctu_rows_arena_layout.restype = i64
    L.ctu_rows_arena_layout.argtypes = [ctypes.POINTER(i64), i32, i32, ctypes.POINTER(i64)]
    L.ctu_engine_run_rows.argtypes = [vp, vp, vp, vp, vp]
    L.ctu_engine_run_rows_host.argtypes = [vp, vp, vp, vp]
    if hasattr(L, "ctu_streams_create"):  # (as above: older builds loaded for an A/B have no stream sets)
        L.ctu_streams_create.argtypes = [vp, i32, i64, ctypes.POINTER(vp)]
        L.ctu_streams_destroy.restype = None
        L.ctu_streams_destroy.argtypes = [vp]
        L.ctu_streams_config_check.argtypes = [ctypes.c_int, argv_t, ctypes.c_char_p, i64]
        L.ctu_streams_push.argtypes = [vp, i32, vp, vp, vp, vp, vp, i64, vp, vp]
        L.ctu_streams_push_host.argtypes = [vp, i32, vp, vp, vp, vp, i64, vp]
        L.ctu_streams_finish.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i64), vp]
        L.ctu_streams_frames.restype = i64
        L.ctu_streams_frames.argtypes = [vp, i32]
        L.ctu_streams_step.restype = i64
        L.ctu_streams_step.argtypes = [i32, i32, i64, ctypes.POINTER(i64)]
        L.ctu_streams_last_push_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    if hasattr(L, "ctu_streams_create_ex"):  # (likewise: stream sets with row state)
        u32 = ctypes.c_uint32
        L.ctu_streams_create_ex.argtypes = [vp, i32, i64, u32, ctypes.POINTER(vp)]
        L.ctu_streams_config_check_ex.argtypes = [ctypes.c_int, argv_t, u32, ctypes.c_char_p, i64, ctypes.POINTER(i32)]
        L.ctu_streams_pending.restype = i64
        L.ctu_streams_pending.argtypes = [vp, i32]
        L.ctu_streams_finish_host.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i64)]
        L.ctu_streams_rows_step.restype = i64
        L.ctu_streams_rows_step.argtypes = [i32, i32, i32, i32, i64, ctypes.POINTER(i64)]
    if hasattr(L, "ctu_streams_vad_step"):  # (likewise: stream sets with detector state)
        L.ctu_streams_push_vad.argtypes = [vp, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp]
        L.ctu_streams_push_vad_host.argtypes = [vp, i32, vp, vp, vp, vp, i64, vp, vp]
        L.ctu_streams_finish_vad.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i64), vp, vp]
        L.ctu_streams_finish_vad_host.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i64), vp]
        L.ctu_streams_vad_step.restype = i64
        L.ctu_streams_vad_step.argtypes = [i32, i32, i32, i64, ctypes.POINTER(i64)]
    if hasattr(L, "ctu_streams_signal_step"):  # (likewise: stream sets with signal state)
        L.ctu_streams_push_signal.argtypes = [vp, i32, vp, vp, vp, vp, vp, i64, vp, vp]
        L.ctu_streams_push_signal_host.argtypes = [vp, i32, vp, vp, vp, vp, i64, vp]
        L.ctu_streams_finish_signal.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i64), vp]
        L.ctu_streams_finish_signal_host.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i64)]
        L.ctu_streams_signal_step.restype = i64
        L.ctu_streams_signal_step.argtypes = [i32, i32, i64, ctypes.POINTER(i64)]
    if hasattr(L, "ctu_streams_vad_rows_step"):  # (likewise: stream sets with detector state behind row state)
        L.ctu_streams_vad_rows_step.restype = i64
        L.ctu_streams_vad_rows_step.argtypes = [i32, i32, i32, i32, i32, i64, ctypes.POINTER(i64)]
    if hasattr(L, "ctu_streams_flags_for"):  # (likewise: the flag set a command line needs)
        L.ctu_streams_flags_for.argtypes = [ctypes.c_int, argv_t, ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, i64, ctypes.POINTER(i32)]
    if hasattr(L, "ctu_streams_push_wire"):  # (likewise: wire input)
        wl = ctypes.POINTER(WireLayout)
        L.ctu_streams_push_wire.argtypes = [vp, i32, vp, vp, vp, vp, wl, vp, i64, vp, vp, vp]
        L.ctu_streams_push_wire_host.argtypes = [vp, i32, vp, vp, vp, vp, wl, vp, i64, vp, vp]
        L.ctu_streams_push_signal_wire.argtypes = [vp, i32, vp, vp, vp, vp, wl, vp, i64, vp, vp]
        L.ctu_streams_push_signal_wire_host.argtypes = [vp, i32, vp, vp, vp, vp, wl, vp, i64, vp]
        L.ctu_wire_extent.restype = i64
        L.ctu_wire_extent.argtypes = [wl, i32, vp, vp, ctypes.POINTER(i64)]
        L.ctu_wire_expand.restype = i64
        L.ctu_wire_expand.argtypes = [wl, vp, i64, i64, vp]
    if hasattr(L, "ctu_plan_unpack_wire"):  # (likewise: wire input of offline runs)
        wl = ctypes.POINTER(WireLayout)
        L.ctu_plan_unpack_wire.argtypes = [vp, vp, vp, vp, wl, vp, vp]
        L.ctu_engine_run_wire_host.argtypes = [vp, vp, vp, vp, wl, vp, vp, vp]
        L.ctu_engine_run_signal_wire_host.argtypes = [vp, vp, vp, vp, wl, vp]
    _lib = L
    return L


def host_alloc(shape, dtype):
    """numpy array over page-locked host memory from ctu_host_alloc (DMA at the link rate in the *_host calls)."""
    L = load_library()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = L.ctu_host_alloc(n)
    if not ptr:
        raise CtuError(CTU_ERR_DEVICE, "ctu_host_alloc failed")
    buf = (ctypes.c_char * n).from_address(ptr)
    # The block lives as long as the ctypes object every derived array ends up holding as its buffer: np.asarray(),
    # np.ascontiguousarray(), slices and .view() of the result all keep `buf` reachable through .base, whatever happens to
    # the first array object (an owner attribute on an ndarray subclass is dropped by those calls while DMA may still run).
    weakref.finalize(buf, L.ctu_host_free, ptr)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def _argv(args):
    args = [str(a).encode() for a in args]
    return len(args), (ctypes.c_char_p * len(args))(*args)


def config_dims(args):
    """Geometry of a command line without touching a GPU (parse + host-side table design)."""
    L = load_library()
    d = Dims()
    n, arr = _argv(args)
    rc = L.ctu_config_dims(n, arr, ctypes.byref(d))
    if rc != CTU_OK:
        raise CtuError(rc, L.ctu_create_error().decode())
    return d


def config_table(args, name):
    """Host-designed table (float64 numpy) by name; see ctu_config_table in include/ctu_engine.h."""
    L = load_library()
    n, arr = _argv(args)
    cnt = L.ctu_config_table(n, arr, name.encode(), None, 0)
    if cnt < 0:
        raise CtuError(int(cnt), L.ctu_create_error().decode())
    out = np.zeros(int(cnt), dtype=np.float64)
    L.ctu_config_table(n, arr, name.encode(), out.ctypes.data, cnt)
    return out


def _stream_flags(row_state=False, nr_state=False, vad_state=False, signal_state=False, large_state=False, trap_state=False, ss_state=False,
                  ss_signal_state=False, ss_large_state=False):
    return ((STREAMS_ROW_STATE if row_state else 0) | (STREAMS_NR_STATE if nr_state else 0) | (STREAMS_VAD_STATE if vad_state else 0) |
            (STREAMS_SIGNAL_STATE if signal_state else 0) | (STREAMS_LARGE_STATE if large_state else 0) |
            (STREAMS_TRAP_STATE if trap_state else 0) | (STREAMS_SS_STATE if ss_state else 0) |
            (STREAMS_SS_SIGNAL_STATE if ss_signal_state else 0) | (STREAMS_SS_LARGE_STATE if ss_large_state else 0))


def streams_config_check(args, row_state=False, nr_state=False, vad_state=False, signal_state=False, large_state=False, trap_state=False,
                         ss_state=False, ss_signal_state=False, ss_large_state=False):
    """(code, reason): whether a command line can be streamed (Engine.streams), without touching a GPU.  CTU_OK and "", or
    CTU_ERR_UNSUPPORTED / CTU_ERR_OPTS and the text ctu_streams_create / ctu_engine_create would give.  With row_state (a set that
    may hold rows back: delta chains, stacking, CMS) the answer is (code, reason, halo).  With nr_state the set keeps the noise
    estimate of -nr_mode exten too, with vad_state the VAD module's detector state, with signal_state the overlap-add's tail of
    speech output (-format_out raw | wave), with large_state exten's estimate and the overlap-add's tail on 1024 .. 4096-point frames.
    With trap_state (a set that keeps the log-mel context of -fea_kind trapdct) the answer is (code, reason, halo) as with row_state:
    the halo is (traplen - 1) / 2.  With ss_state the set keeps what -nr_mode hwss | fwss | 2fwss carry along a file (noise estimates and
    the Burg-cepstral detector's record); with ss_signal_state beside ss_state and signal_state, the set streams the speech output of
    those modes; with ss_large_state beside ss_state the feature path of those modes reaches 2048- and 4096-point frames.
    The flag that has no keyword here, STREAMS_VAD_ROW_STATE, is asked with streams_config_check_ex."""
    L = load_library()
    n, arr = _argv(args)
    buf = ctypes.create_string_buffer(1024)
    halo = ctypes.c_int32(0)  # (no flag set: flags 0, which is all the plain ctu_streams_config_check passes on)
    flags = _stream_flags(row_state, nr_state, vad_state, signal_state, large_state, trap_state, ss_state, ss_signal_state, ss_large_state)
    rc = L.ctu_streams_config_check_ex(n, arr, flags, buf, len(buf), ctypes.byref(halo))
    return (int(rc), buf.value.decode(), int(halo.value)) if row_state or trap_state else (int(rc), buf.value.decode())


def streams_config_check_ex(args, flags):
    """(code, reason, halo) of a command line for a stream set created with the STREAMS_* bits `flags` (Engine.streams_ex), without
    touching a GPU: ctu_streams_config_check_ex as it stands.  The keywords of streams_config_check are the bits up to
    STREAMS_SS_LARGE_STATE; STREAMS_VAD_ROW_STATE - beside STREAMS_ROW_STATE and STREAMS_VAD_STATE the VAD module with delta chains,
    stacking and CMS behind it, the halo the chain's plus (vad_filter_order - 1) / 2 - is given here."""
    L = load_library()
    n, arr = _argv(args)
    buf = ctypes.create_string_buffer(1024)
    halo = ctypes.c_int32(0)
    rc = L.ctu_streams_config_check_ex(n, arr, int(flags), buf, len(buf), ctypes.byref(halo))
    return int(rc), buf.value.decode(), int(halo.value)


def streams_flags_for(args):
    """(code, flags, reason, halo): the STREAMS_* bits a command line needs on a stream set (ctu_streams_flags_for), without touching a
    GPU, and what streams_config_check_ex(args, flags) answers for them - CTU_OK, "" and the halo, or the refusal of that set.  The
    flags are given in both outcomes (0 behind a command line the parser refuses)."""
    L = load_library()
    n, arr = _argv(args)
    buf = ctypes.create_string_buffer(1024)
    flags, halo = ctypes.c_uint32(0), ctypes.c_int32(0)
    rc = L.ctu_streams_flags_for(n, arr, ctypes.byref(flags), buf, len(buf), ctypes.byref(halo))
    return int(rc), int(flags.value), buf.value.decode(), int(halo.value)


def streams_step(window, wshift, total):
    """(frames produced, samples the next frame already has) of a stream after `total` samples (ctu_streams_step)."""
    carry = ctypes.c_int64(0)
    f = load_library().ctu_streams_step(int(window), int(wshift), int(total), ctypes.byref(carry))
    if f < 0:
        raise CtuError(int(f), "ctu_streams_step: bad argument")
    return int(f), int(carry.value)


def streams_rows_step(window, wshift, halo, wmax, total):
    """(rows delivered, rows held back) of a stream with row state after `total` samples, for a chain of halo `halo` and largest
    window `wmax` (ctu_streams_rows_step)."""
    pending = ctypes.c_int64(0)
    r = load_library().ctu_streams_rows_step(int(window), int(wshift), int(halo), int(wmax), int(total), ctypes.byref(pending))
    if r < 0:
        raise CtuError(int(r), "ctu_streams_rows_step: bad argument")
    return int(r), int(pending.value)


def streams_vad_step(window, wshift, filter_order, total):
    """(rows and decisions delivered, frames held back) of a stream with detector state after `total` samples, for a majority filter
    of order `filter_order` (ctu_streams_vad_step)."""
    pending = ctypes.c_int64(0)
    r = load_library().ctu_streams_vad_step(int(window), int(wshift), int(filter_order), int(total), ctypes.byref(pending))
    if r < 0:
        raise CtuError(int(r), "ctu_streams_vad_step: bad argument")
    return int(r), int(pending.value)


def streams_vad_rows_step(window, wshift, filter_order, halo, wmax, total):
    """(rows and decisions delivered, frames held back) of a stream with detector state behind row state after `total` samples: a chain
    of halo `halo` and largest window `wmax` ahead of a majority filter of order `filter_order` (ctu_streams_vad_rows_step)."""
    pending = ctypes.c_int64(0)
    r = load_library().ctu_streams_vad_rows_step(int(window), int(wshift), int(filter_order), int(halo), int(wmax), int(total), ctypes.byref(pending))
    if r < 0:
        raise CtuError(int(r), "ctu_streams_vad_rows_step: bad argument")
    return int(r), int(pending.value)


def streams_signal_step(window, wshift, total):
    """(samples delivered, samples a finish adds) of a stream with signal state after `total` input samples (ctu_streams_signal_step)."""
    pending = ctypes.c_int64(0)
    r = load_library().ctu_streams_signal_step(int(window), int(wshift), int(total), ctypes.byref(pending))
    if r < 0:
        raise CtuError(int(r), "ctu_streams_signal_step: bad argument")
    return int(r), int(pending.value)


def _wire_layout(fmt, stride):
    """The ctu_wire_layout of a format name (or CTU_WIRE_* number) and a stride; what the library refuses is passed on as it is."""
    return WireLayout(int(WIRE_FORMATS.get(fmt, fmt) if isinstance(fmt, str) else fmt), int(stride))


def _wire_elem_dtype(fmt):
    return np.uint8 if WIRE_FORMATS.get(fmt, fmt) in (2, 3) else np.int16


def wire_extent(elem_off, n_samples, fmt="s16", stride=1):
    """(elements, first element) of the covering range of a push (ctu_wire_extent): from the lowest element any stream reads to the
    highest; (0, 0) for a push without samples."""
    off = np.ascontiguousarray(elem_off, dtype=np.int64)
    ns = np.ascontiguousarray(n_samples, dtype=np.int64)
    assert off.size == ns.size
    w, first = _wire_layout(fmt, stride), ctypes.c_int64(0)
    r = load_library().ctu_wire_extent(ctypes.byref(w), int(ns.size), off.ctypes.data, ns.ctypes.data, ctypes.byref(first))
    if r < 0:
        raise CtuError(int(r), "ctu_wire_extent: bad argument")
    return int(r), int(first.value)


def wire_expand(buf, elem_off, n_samples, fmt="s16", stride=1):
    """int16 [n_samples]: the samples of a stream whose first is element `elem_off` of the numpy buffer `buf` (ctu_wire_expand)."""
    buf = np.ascontiguousarray(buf)
    w = _wire_layout(fmt, stride)
    n, e0 = int(n_samples), int(elem_off)
    if n > 0 and e0 >= 0 and w.stride >= 1:
        assert (e0 + (n - 1) * w.stride + 1) * np.dtype(_wire_elem_dtype(fmt)).itemsize <= buf.nbytes
    out = np.empty(max(n, 0), dtype=np.int16)
    r = load_library().ctu_wire_expand(ctypes.byref(w), buf.ctypes.data, e0, n, out.ctypes.data)
    if r < 0:
        raise CtuError(int(r), "ctu_wire_expand: bad argument")
    return out[:int(r)]


class Streams:
    """A set of `n` streams on an engine (Engine.streams): PCM in per stream as it arrives, the rows of the frames it completes out.
    With row_state the set takes delta chains, stacking and CMS too, and may deliver a frame's row with a later push or with finish.
    With nr_state it takes -nr_mode exten (on the spectrum, 256- and 512-point front end): the noise estimate is kept per stream.
    With vad_state it takes the VAD module (energy and Burg-cepstral criteria): the detector's state is kept per stream, and a frame's
    row leaves with its decision, (vad_filter_order - 1) / 2 frames late.
    With signal_state it takes speech output (-format_out raw | wave; with nr_state as well behind -nr_mode exten): push_signal and
    finish_signal deliver the enhanced samples, wshift per completed frame and the window - wshift behind them at the file's end.
    With large_state, nr_state and signal_state reach 1024 .. 4096-point frames too (exten on the spectrum, speech output); it is a
    flag beside one of the two only.
    With trap_state it takes -fea_kind trapdct (the plain chain, and with nr_state behind -nr_mode exten): the last traplen - 1 log-mel
    rows are kept per stream, a frame's row leaves (traplen - 1) / 2 frames late and finish delivers the last (traplen - 1) / 2.
    With ss_state it takes -nr_mode hwss | fwss | 2fwss with -vad burg on the feature path of the 256- and 512-point front end: the noise
    estimates and the detector's record are kept per stream, and every file of a stream gives the rows of a fresh engine's extract of it.
    With ss_signal_state beside ss_state and signal_state it takes those modes with speech output (-format_out raw | wave): push_signal
    and finish_signal deliver the samples of a fresh engine's enhance of the file.
    With ss_large_state beside ss_state it takes those modes with -vad burg on the feature path of 2048- and 4096-point frames (44.1 /
    48 kHz audio): both estimates and the detector's record are kept per stream in double, as the large transforms' kernels hold them.
    Streams.with_flags (Engine.streams_ex) creates a set from the STREAMS_* bits themselves.  With STREAMS_VAD_ROW_STATE beside
    STREAMS_ROW_STATE and STREAMS_VAD_STATE it takes the VAD module with delta chains, stacking and CMS behind it: the detector is called
    when a chain row is complete, and a row leaves with its decision (vad_filter_order - 1) / 2 calls later or with finish."""

    def __init__(self, engine, n, max_push, row_state=False, nr_state=False, vad_state=False, signal_state=False, large_state=False,
                 trap_state=False, ss_state=False, ss_signal_state=False, ss_large_state=False):
        self._create(engine, n, max_push, _stream_flags(row_state, nr_state, vad_state, signal_state, large_state, trap_state, ss_state, ss_signal_state,
                                                        ss_large_state))

    @classmethod
    def with_flags(cls, engine, n, max_push, flags):
        """A set created with the STREAMS_* bits `flags` (ctu_streams_create_ex as it stands)."""
        st = cls.__new__(cls)
        st._create(engine, n, max_push, int(flags))
        return st

    def _create(self, engine, n, max_push, flags):
        L = load_library()
        self.engine, self.n, self.max_push = engine, int(n), int(max_push)
        h = ctypes.c_void_p()
        rc = L.ctu_streams_create_ex(engine._h, self.n, self.max_push, flags, ctypes.byref(h))  # (flags 0: what the plain ctu_streams_create passes on)
        if rc != CTU_OK:
            raise CtuError(rc, L.ctu_last_error(engine._h).decode())
        self._h = h
        engine._sets.add(h.value)

    def close(self):
        # ctu_streams_destroy reads its engine, so a set must go first.  The collector finalises the objects of a reference cycle in
        # any order (a caught CtuError's traceback makes such cycles): the engine destroys the sets it still knows of ahead of itself
        # (Engine.close), and a set that finds its handle gone from the engine's books has nothing left to destroy.
        h, self._h = getattr(self, "_h", None), None
        if h and h.value in self.engine._sets:
            self.engine._sets.discard(h.value)
            load_library().ctu_streams_destroy(h)

    __del__ = close

    def push(self, chunks, want_vad=False):
        """{stream id: int16 array} -> {stream id: float32 [rows, D]}: the frames the new samples complete (host buffers).
        With want_vad (a set with detector state): {stream id: (rows, uint8 [rows] decisions '0' / '1')}."""
        ids = np.array(list(chunks.keys()), dtype=np.int32)
        arrs = [np.ascontiguousarray(chunks[k], dtype=np.int16).reshape(-1) for k in chunks]
        ns = np.array([a.size for a in arrs], dtype=np.int64)
        ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        D = self.engine.dims.row_floats
        sh = self.engine.dims.wshift
        # at most one frame more than whole hops per stream, and what the stream held back
        cap = int(sum(int(a) // sh + 1 + self.pending(int(k)) for k, a in zip(ids, ns) if 0 <= k < self.n))
        rows = np.empty((cap, D), dtype=np.float32)
        counts = np.zeros(max(len(arrs), 1), dtype=np.int64)
        if want_vad:
            vad = np.zeros(max(cap, 1), dtype=np.uint8)
            rc = load_library().ctu_streams_push_vad_host(self._h, len(arrs), ids.ctypes.data, ptrs, ns.ctypes.data, rows.ctypes.data, cap, counts.ctypes.data,
                                                          vad.ctypes.data)
        else:
            rc = load_library().ctu_streams_push_host(self._h, len(arrs), ids.ctypes.data, ptrs, ns.ctypes.data, rows.ctypes.data, cap, counts.ctypes.data)
        self.engine._check(rc)
        out, at = {}, 0
        for k, c in zip(chunks, counts):
            out[k] = (rows[at:at + int(c)], vad[at:at + int(c)]) if want_vad else rows[at:at + int(c)]
            at += int(c)
        return out

    def push_device(self, ids, pcm, sample_off, n_samples, rows, stream=None, vad=None):
        """Device form: pcm a torch int16 CUDA tensor holding stream ids[i]'s n_samples[i] new samples at sample_off[i]; rows a float32
        CUDA tensor [capacity, D]; vad (a set with detector state) a uint8 CUDA tensor [capacity] for the rows' decisions.  Returns the
        row counts per stream (numpy int64); asynchronous on `stream`."""
        import torch
        assert pcm.is_cuda and pcm.dtype == torch.int16 and rows.is_cuda and rows.dtype == torch.float32
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        off = np.ascontiguousarray(sample_off, dtype=np.int64)
        ns = np.ascontiguousarray(n_samples, dtype=np.int64)
        assert ids.size == off.size == ns.size and (ns.size == 0 or int((off + ns).max()) <= pcm.numel())
        counts = np.zeros(max(ids.size, 1), dtype=np.int64)
        s = stream if stream is not None else torch.cuda.current_stream(pcm.device)
        cap = rows.numel() // self.engine.dims.row_floats
        if vad is not None:
            assert vad.is_cuda and vad.dtype == torch.uint8 and vad.numel() >= cap
            self.engine._check(load_library().ctu_streams_push_vad(self._h, int(ids.size), ids.ctypes.data, pcm.data_ptr(), off.ctypes.data, ns.ctypes.data,
                                                                   rows.data_ptr(), cap, counts.ctypes.data, vad.data_ptr(), s.cuda_stream))
            return counts[:ids.size]
        self.engine._check(load_library().ctu_streams_push(self._h, int(ids.size), ids.ctypes.data, pcm.data_ptr(), off.ctypes.data, ns.ctypes.data,
                                                           rows.data_ptr(), cap, counts.ctypes.data, s.cuda_stream))
        return counts[:ids.size]

    def finish(self, sid, want_vad=False):
        """Ends stream `sid`'s file: its remaining rows - the ones a set with row or detector state held back, else [0, D]: the reference
        makes no frame of a trailing partial window; the stream then starts a new file.  With want_vad: (rows, their decisions)."""
        cnt = ctypes.c_int64(0)
        cap = max(self.pending(sid), 0)
        rows = np.empty((cap, self.engine.dims.row_floats), dtype=np.float32)
        if want_vad:
            vad = np.zeros(max(cap, 1), dtype=np.uint8)
            self.engine._check(load_library().ctu_streams_finish_vad_host(self._h, int(sid), rows.ctypes.data if cap else None, cap, ctypes.byref(cnt),
                                                                          vad.ctypes.data))
            return rows[:int(cnt.value)], vad[:int(cnt.value)]
        self.engine._check(load_library().ctu_streams_finish_host(self._h, int(sid), rows.ctypes.data if cap else None, cap, ctypes.byref(cnt)))
        return rows[:int(cnt.value)]

    def finish_device(self, sid, rows, vad=None, stream=None):
        """Device form of finish: rows a float32 CUDA tensor [capacity, D] for the rows held back, vad (a set with detector state) a uint8
        CUDA tensor [capacity] for their decisions.  Returns the row count; asynchronous on `stream`."""
        import torch
        assert rows.is_cuda and rows.dtype == torch.float32
        cnt = ctypes.c_int64(0)
        s = stream if stream is not None else torch.cuda.current_stream(rows.device)
        cap = rows.numel() // self.engine.dims.row_floats
        if vad is not None:
            assert vad.is_cuda and vad.dtype == torch.uint8 and vad.numel() >= cap
            self.engine._check(load_library().ctu_streams_finish_vad(self._h, int(sid), rows.data_ptr(), cap, ctypes.byref(cnt), vad.data_ptr(), s.cuda_stream))
        else:
            self.engine._check(load_library().ctu_streams_finish(self._h, int(sid), rows.data_ptr(), cap, ctypes.byref(cnt), s.cuda_stream))
        return int(cnt.value)

    def push_signal(self, chunks, capacity=None):
        """{stream id: int16 array} -> {stream id: int16 array}: the enhanced samples the new input completes, wshift for every frame
        (a set with signal_state; host buffers).  `capacity`: the room offered for them (default: enough for any such push)."""
        ids = np.array(list(chunks.keys()), dtype=np.int32)
        arrs = [np.ascontiguousarray(chunks[k], dtype=np.int16).reshape(-1) for k in chunks]
        ns = np.array([a.size for a in arrs], dtype=np.int64)
        ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        sh = self.engine.dims.wshift
        cap = int(sum((int(a) // sh + 1) * sh for a in ns)) if capacity is None else int(capacity)  # at most one frame more than whole hops per stream
        out = np.empty(max(cap, 1), dtype=np.int16)
        counts = np.zeros(max(len(arrs), 1), dtype=np.int64)
        self.engine._check(load_library().ctu_streams_push_signal_host(self._h, len(arrs), ids.ctypes.data, ptrs, ns.ctypes.data, out.ctypes.data, cap,
                                                                       counts.ctypes.data))
        res, at = {}, 0
        for k, c in zip(chunks, counts):
            res[k] = out[at:at + int(c)]
            at += int(c)
        return res

    def push_signal_device(self, ids, pcm, sample_off, n_samples, out, stream=None):
        """Device form: pcm as in push_device; out a torch int16 CUDA tensor for the samples.  Returns the sample counts per stream
        (numpy int64); asynchronous on `stream`."""
        import torch
        assert pcm.is_cuda and pcm.dtype == torch.int16 and out.is_cuda and out.dtype == torch.int16
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        off = np.ascontiguousarray(sample_off, dtype=np.int64)
        ns = np.ascontiguousarray(n_samples, dtype=np.int64)
        assert ids.size == off.size == ns.size and (ns.size == 0 or int((off + ns).max()) <= pcm.numel())
        counts = np.zeros(max(ids.size, 1), dtype=np.int64)
        s = stream if stream is not None else torch.cuda.current_stream(pcm.device)
        self.engine._check(load_library().ctu_streams_push_signal(self._h, int(ids.size), ids.ctypes.data, pcm.data_ptr(), off.ctypes.data, ns.ctypes.data,
                                                                  out.data_ptr(), out.numel(), counts.ctypes.data, s.cuda_stream))
        return counts[:ids.size]

    def finish_signal(self, sid):
        """Ends stream `sid`'s file on a set with signal_state: the window - wshift samples behind the ones delivered (none for a file
        without a frame); the stream then starts a new file."""
        cnt = ctypes.c_int64(0)
        cap = max(self.pending(sid), 0)
        out = np.empty(max(cap, 1), dtype=np.int16)
        self.engine._check(load_library().ctu_streams_finish_signal_host(self._h, int(sid), out.ctypes.data if cap else None, cap, ctypes.byref(cnt)))
        return out[:int(cnt.value)]

    def finish_signal_device(self, sid, out, stream=None):
        """Device form of finish_signal: out a torch int16 CUDA tensor for the tail's samples.  Returns the sample count; asynchronous on
        `stream`."""
        import torch
        assert out.is_cuda and out.dtype == torch.int16
        cnt = ctypes.c_int64(0)
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        self.engine._check(load_library().ctu_streams_finish_signal(self._h, int(sid), out.data_ptr(), out.numel(), ctypes.byref(cnt), s.cuda_stream))
        return int(cnt.value)

    # ---- wire input: G.711 codes, swapped and channel-interleaved PCM as they lie in one buffer (ctu_streams_push_wire*)
    def _wire_args(self, ids, elem_off, n_samples, fmt, stride, nbytes):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        off = np.ascontiguousarray(elem_off, dtype=np.int64)
        ns = np.ascontiguousarray(n_samples, dtype=np.int64)
        w = _wire_layout(fmt, stride)
        assert ids.size == off.size == ns.size
        live = ns > 0
        if w.stride >= 1 and live.any() and (off[live] >= 0).all():  # (what the library refuses is the library's to refuse)
            last = int((off[live] + (ns[live] - 1) * w.stride).max())
            assert (last + 1) * np.dtype(_wire_elem_dtype(w.format)).itemsize <= nbytes, "the layout reads past the buffer"
        return ids, off, ns, w

    def _split(self, ids, counts, *arrays):
        out, at = {}, 0
        for k, c in zip(ids.tolist(), counts):
            part = tuple(a[at:at + int(c)] for a in arrays)
            out[k] = part if len(part) > 1 else part[0]
            at += int(c)
        return out

    def push_wire(self, buf, ids, elem_off, n_samples, fmt="s16", stride=1, want_vad=False):
        """Host form of a wire push: `buf` one numpy buffer (pageable, or page-locked from host_alloc) of int16 / uint8 elements; sample k
        of stream ids[i] is element elem_off[i] + k * stride of it, expanded by `fmt` ("s16", "s16_swapped", "alaw", "mulaw").  Returns
        what push returns: {stream id: float32 [rows, D]}, with want_vad {stream id: (rows, decisions)}."""
        buf = np.asarray(buf)
        assert buf.flags["C_CONTIGUOUS"]
        ids, off, ns, w = self._wire_args(ids, elem_off, n_samples, fmt, stride, buf.nbytes)
        D, sh = self.engine.dims.row_floats, self.engine.dims.wshift
        cap = int(sum(int(a) // sh + 1 + self.pending(int(k)) for k, a in zip(ids, ns) if 0 <= k < self.n and a >= 0))
        rows = np.empty((cap, D), dtype=np.float32)
        vad = np.zeros(max(cap, 1), dtype=np.uint8)
        counts = np.zeros(max(ids.size, 1), dtype=np.int64)
        self.engine._check(load_library().ctu_streams_push_wire_host(self._h, int(ids.size), ids.ctypes.data, buf.ctypes.data, off.ctypes.data, ns.ctypes.data,
                                                                     ctypes.byref(w), rows.ctypes.data, cap, counts.ctypes.data,
                                                                     vad.ctypes.data if want_vad else None))
        return self._split(ids, counts, rows, vad) if want_vad else self._split(ids, counts, rows)

    def push_wire_device(self, ids, buf, elem_off, n_samples, rows, fmt="s16", stride=1, stream=None, vad=None):
        """Device form: buf a torch CUDA tensor (int16 or uint8 elements) read as push_wire reads its buffer; rows, vad and the result as
        in push_device."""
        import torch
        assert buf.is_cuda and buf.is_contiguous() and rows.is_cuda and rows.dtype == torch.float32
        ids, off, ns, w = self._wire_args(ids, elem_off, n_samples, fmt, stride, buf.numel() * buf.element_size())
        counts = np.zeros(max(ids.size, 1), dtype=np.int64)
        s = stream if stream is not None else torch.cuda.current_stream(buf.device)
        cap = rows.numel() // self.engine.dims.row_floats
        if vad is not None:
            assert vad.is_cuda and vad.dtype == torch.uint8 and vad.numel() >= cap
        self.engine._check(load_library().ctu_streams_push_wire(self._h, int(ids.size), ids.ctypes.data, buf.data_ptr(), off.ctypes.data, ns.ctypes.data,
                                                                ctypes.byref(w), rows.data_ptr(), cap, counts.ctypes.data,
                                                                vad.data_ptr() if vad is not None else None, s.cuda_stream))
        return counts[:ids.size]

    def push_signal_wire(self, buf, ids, elem_off, n_samples, fmt="s16", stride=1, capacity=None):
        """Host form of a wire push on a set with signal_state: the buffer as in push_wire, the result as push_signal's."""
        buf = np.asarray(buf)
        assert buf.flags["C_CONTIGUOUS"]
        ids, off, ns, w = self._wire_args(ids, elem_off, n_samples, fmt, stride, buf.nbytes)
        sh = self.engine.dims.wshift
        cap = int(sum((int(a) // sh + 1) * sh for a in ns if a >= 0)) if capacity is None else int(capacity)
        out = np.empty(max(cap, 1), dtype=np.int16)
        counts = np.zeros(max(ids.size, 1), dtype=np.int64)
        self.engine._check(load_library().ctu_streams_push_signal_wire_host(self._h, int(ids.size), ids.ctypes.data, buf.ctypes.data, off.ctypes.data,
                                                                            ns.ctypes.data, ctypes.byref(w), out.ctypes.data, cap, counts.ctypes.data))
        return self._split(ids, counts, out)

    def push_signal_wire_device(self, ids, buf, elem_off, n_samples, out, fmt="s16", stride=1, stream=None):
        """Device form: buf as in push_wire_device, out and the result as in push_signal_device."""
        import torch
        assert buf.is_cuda and buf.is_contiguous() and out.is_cuda and out.dtype == torch.int16
        ids, off, ns, w = self._wire_args(ids, elem_off, n_samples, fmt, stride, buf.numel() * buf.element_size())
        counts = np.zeros(max(ids.size, 1), dtype=np.int64)
        s = stream if stream is not None else torch.cuda.current_stream(buf.device)
        self.engine._check(load_library().ctu_streams_push_signal_wire(self._h, int(ids.size), ids.ctypes.data, buf.data_ptr(), off.ctypes.data, ns.ctypes.data,
                                                                       ctypes.byref(w), out.data_ptr(), out.numel(), counts.ctypes.data, s.cuda_stream))
        return counts[:ids.size]

    def push_interleaved(self, frames, ids=None, fmt="s16", want_vad=False):
        """A [samples, channels] numpy block as capture hardware delivers it: channel j goes to stream ids[j] (default j), all of its
        samples.  One buffer, one upload (push_wire with stride = channels, elem_off = j)."""
        frames = np.asarray(frames)
        assert frames.ndim == 2 and frames.flags["C_CONTIGUOUS"]
        samples, channels = frames.shape
        ids = np.arange(channels, dtype=np.int32) if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        assert ids.size == channels
        return self.push_wire(frames, ids, np.arange(channels, dtype=np.int64), np.full(channels, samples, dtype=np.int64), fmt=fmt, stride=channels,
                              want_vad=want_vad)

    def frames(self, sid):
        """Rows of the current file delivered so far."""
        return int(load_library().ctu_streams_frames(self._h, int(sid)))

    def pending(self, sid):
        """Rows a finish would deliver now."""
        return int(load_library().ctu_streams_pending(self._h, int(sid)))

    def last_push_ms(self):
        """(stream_stitch_kernel, front end and tails, stream_carry_kernel) of the last push, in ms (HIP events)."""
        ms = (ctypes.c_float * 3)()
        self.engine._check(load_library().ctu_streams_last_push_ms(self._h, ms))
        return tuple(float(x) for x in ms)


class Plan:
    """Batch layout: where each utterance sits in the packed PCM arena and in the output rows."""

    def __init__(self, engine, nsamples):
        L = load_library()
        self.engine = engine
        ns = np.ascontiguousarray(nsamples, dtype=np.int64)
        self.n_utt = int(ns.size)
        h = ctypes.c_void_p()
        rc = L.ctu_plan_create(engine._h, ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), self.n_utt, ctypes.byref(h))
        if rc != CTU_OK:
            raise CtuError(rc, L.ctu_last_error(engine._h).decode())
        self._h = h
        self.nsamples = ns
        self.sample_off = np.ctypeslib.as_array(L.ctu_plan_sample_offsets(h), shape=(self.n_utt + 1,)).copy()
        self.row_off = np.ctypeslib.as_array(L.ctu_plan_row_offsets(h), shape=(self.n_utt + 1,)).copy()
        self.total_samples = int(L.ctu_plan_total_samples(h))
        self.total_frames = int(L.ctu_plan_total_frames(h))

    def set_vad_ring(self, hidx):
        """The historyIdx of the VAD's majority filter every utterance starts with (None: all in phase): the reference's list behaviour,
        see include/ctu_engine.h."""
        L = load_library()
        if hidx is None:
            rc = L.ctu_plan_set_vad_ring(self._h, None)
        else:
            a = np.ascontiguousarray(hidx, dtype=np.int32)
            assert a.size == self.n_utt
            rc = L.ctu_plan_set_vad_ring(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        if rc != CTU_OK:
            raise CtuError(rc, L.ctu_last_error(self.engine._h).decode())

    def pack(self, utterances):
        """int16 arena (numpy) holding the utterances at their planned offsets."""
        arena = np.zeros(self.total_samples, dtype=np.int16)
        for u, off in zip(utterances, self.sample_off[:-1]):
            arena[off:off + len(u)] = u
        return arena

    def close(self):
        if getattr(self, "_h", None):
            load_library().ctu_plan_destroy(self._h)
            self._h = None

    __del__ = close


class Engine:
    """One configured chain on one GPU; `args` is the ctucopy command line (list of str)."""

    def __init__(self, args, device=0):
        L = load_library()
        n, arr = _argv(args)
        h = ctypes.c_void_p()
        rc = L.ctu_engine_create(n, arr, int(device), ctypes.byref(h))
        if rc != CTU_OK:
            raise CtuError(rc, L.ctu_create_error().decode())
        self._h = h
        self._sets = set()  # handles of the live stream sets on this engine (Streams)
        self.device = int(device)
        self.dims = Dims()
        L.ctu_engine_dims(h, ctypes.byref(self.dims))

    def close(self):
        if getattr(self, "_h", None):
            L = load_library()
            while getattr(self, "_sets", None):  # a stream set is destroyed ahead of its engine (see Streams.close)
                L.ctu_streams_destroy(ctypes.c_void_p(self._sets.pop()))
            L.ctu_engine_destroy(self._h)
            self._h = None

    __del__ = close

    def num_frames(self, nsamples):
        return int(load_library().ctu_num_frames(self._h, int(nsamples)))

    def plan(self, nsamples):
        return Plan(self, nsamples)

    def streams(self, n, max_push, row_state=False, nr_state=False, vad_state=False, signal_state=False, large_state=False, trap_state=False,
                ss_state=False, ss_signal_state=False, ss_large_state=False):
        """A set of n streams taking up to max_push samples per stream and push (see Streams)."""
        return Streams(self, n, max_push, row_state, nr_state, vad_state, signal_state, large_state, trap_state, ss_state, ss_signal_state, ss_large_state)

    def streams_ex(self, n, max_push, flags):
        """The same from the STREAMS_* bits themselves (Streams.with_flags): how a set with STREAMS_VAD_ROW_STATE is created."""
        return Streams.with_flags(self, n, max_push, flags)

    def _check(self, rc):
        if rc != CTU_OK:
            raise CtuError(rc, load_library().ctu_last_error(self._h).decode())

    def run_device(self, plan, pcm, rows=None, vad=None, stream=None):
        """pcm: torch int16 CUDA tensor [plan.total_samples]; returns the float32 rows tensor (async)."""
        import torch
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.numel() >= plan.total_samples
        if rows is None:
            rows = torch.empty((plan.total_frames, self.dims.row_floats), dtype=torch.float32, device=pcm.device)
        s = stream if stream is not None else torch.cuda.current_stream(pcm.device)
        self._check(load_library().ctu_engine_run(self._h, plan._h, pcm.data_ptr(), rows.data_ptr(),
                                                  vad.data_ptr() if vad is not None else None, s.cuda_stream))
        return rows

    def run_host(self, plan, arena, want_vad=False, rows_out=None):
        """numpy int16 arena in, numpy float32 rows out (H2D + kernels + D2H inside the library).

        With want_vad: (rows, vad bytes '0'/'1' per frame, rows actually kept per utterance)."""
        arena = np.ascontiguousarray(arena, dtype=np.int16)
        assert arena.size >= plan.total_samples
        rows = rows_out if rows_out is not None else np.empty((plan.total_frames, self.dims.row_floats), dtype=np.float32)
        per = np.zeros(plan.n_utt, dtype=np.int64)
        vad = np.zeros(max(plan.total_frames, 1), dtype=np.uint8)
        self._check(load_library().ctu_engine_run_host(self._h, plan._h, arena.ctypes.data, rows.ctypes.data,
                                                       vad.ctypes.data if self.dims.has_vad else None, per.ctypes.data))
        if want_vad:
            return rows, vad[:plan.total_frames], per
        return rows

    # ---- speech enhancement output (-format_out raw|wave)
    def enhance(self, utterances):
        """list of int16 arrays -> list of int16 arrays (frames*wshift + window-wshift samples each)."""
        L = load_library()
        plan = self.plan([len(u) for u in utterances])
        arena = plan.pack(utterances)
        out = np.zeros(plan.total_samples, dtype=np.int16)
        self._check(L.ctu_engine_run_signal_host(self._h, plan._h, arena.ctypes.data, out.ctypes.data))
        n = L.ctu_plan_out_samples(plan._h)
        res = [out[plan.sample_off[i]:plan.sample_off[i] + n[i]].copy() for i in range(plan.n_utt)]
        plan.close()
        return res

    def enhance_device(self, plan, pcm, out=None, stream=None):
        """pcm: torch int16 CUDA tensor [plan.total_samples] -> int16 CUDA tensor of the same layout (async)."""
        import torch
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.numel() >= plan.total_samples
        if out is None:
            out = torch.zeros(plan.total_samples, dtype=torch.int16, device=pcm.device)
        s = stream if stream is not None else torch.cuda.current_stream(pcm.device)
        self._check(load_library().ctu_engine_run_signal(self._h, plan._h, pcm.data_ptr(), out.data_ptr(), s.cuda_stream))
        return out

    # ---- wire input of offline runs: G.711 codes, swapped and channel-interleaved PCM as they lie in one buffer (ctu_plan_unpack_wire)
    def _wire_plan_args(self, plan, elem_off, fmt, stride, nbytes):
        off = np.ascontiguousarray(elem_off, dtype=np.int64)
        w = _wire_layout(fmt, stride)
        assert off.size == plan.n_utt
        live = plan.nsamples > 0
        if w.stride >= 1 and w.format in WIRE_FORMATS.values() and live.any() and (off[live] >= 0).all():  # (what the library refuses is the library's to refuse)
            last = (off[live].astype(object) + (plan.nsamples[live].astype(object) - 1) * w.stride).max()
            if last < 2 ** 62:
                assert (int(last) + 1) * np.dtype(_wire_elem_dtype(w.format)).itemsize <= nbytes, "the layout reads past the buffer"
        return off, w

    def unpack_wire_device(self, plan, buf, elem_off, fmt="s16", stride=1, pcm=None, stream=None):
        """buf: torch CUDA tensor of int16 / uint8 elements; sample k of utterance i of `plan` is element elem_off[i] + k * stride of it,
        expanded by `fmt` ("s16", "s16_swapped", "alaw", "mulaw") into the plan's arena `pcm` (torch int16 CUDA tensor
        [plan.total_samples], made when None; only the utterances' samples are written).  Returns pcm (async): run_device /
        enhance_device take it."""
        import torch
        assert buf.is_cuda and buf.is_contiguous()
        off, w = self._wire_plan_args(plan, elem_off, fmt, stride, buf.numel() * buf.element_size())
        if pcm is None:
            pcm = torch.zeros(plan.total_samples, dtype=torch.int16, device=buf.device)
        assert pcm.is_cuda and pcm.dtype == torch.int16 and pcm.numel() >= plan.total_samples
        s = stream if stream is not None else torch.cuda.current_stream(buf.device)
        self._check(load_library().ctu_plan_unpack_wire(self._h, plan._h, buf.data_ptr(), off.ctypes.data, ctypes.byref(w), pcm.data_ptr(),
                                                        s.cuda_stream))
        return pcm

    def run_wire_host(self, plan, buf, elem_off, fmt="s16", stride=1, want_vad=False, rows_out=None):
        """run_host with the utterances read out of the numpy buffer `buf` (pageable, or page-locked from host_alloc) through a wire
        layout (ctu_engine_run_wire_host): the wire bytes go up, the device expands them."""
        buf = np.asarray(buf)
        assert buf.flags["C_CONTIGUOUS"]
        off, w = self._wire_plan_args(plan, elem_off, fmt, stride, buf.nbytes)
        rows = rows_out if rows_out is not None else np.empty((plan.total_frames, self.dims.row_floats), dtype=np.float32)
        per = np.zeros(plan.n_utt, dtype=np.int64)
        vad = np.zeros(max(plan.total_frames, 1), dtype=np.uint8)
        self._check(load_library().ctu_engine_run_wire_host(self._h, plan._h, buf.ctypes.data, off.ctypes.data, ctypes.byref(w), rows.ctypes.data,
                                                            vad.ctypes.data if self.dims.has_vad else None, per.ctypes.data))
        if want_vad:
            return rows, vad[:plan.total_frames], per
        return rows

    def extract_wire(self, buf, elem_off, n_samples, fmt="s16", stride=1, want_vad=False):
        """extract with utterance i the n_samples[i] samples that start at element elem_off[i] of `buf`, `stride` elements apart: list of
        [rows, D] float32 arrays (and the VAD byte strings)."""
        plan = self.plan(n_samples)
        rows, vad, per = self.run_wire_host(plan, buf, elem_off, fmt=fmt, stride=stride, want_vad=True)
        out = [rows[plan.row_off[i]:plan.row_off[i] + per[i]] for i in range(plan.n_utt)]
        vads = [vad[plan.row_off[i]:plan.row_off[i + 1]] for i in range(plan.n_utt)]
        vads = [v[v != 0] for v in vads]  # NUL = nothing written (an utterance the majority filter never got ready on)
        plan.close()
        return (out, vads) if want_vad else out

    def enhance_wire(self, buf, elem_off, n_samples, fmt="s16", stride=1):
        """enhance with the utterances read as in extract_wire (ctu_engine_run_signal_wire_host): list of int16 arrays."""
        L = load_library()
        buf = np.asarray(buf)
        assert buf.flags["C_CONTIGUOUS"]
        plan = self.plan(n_samples)
        off, w = self._wire_plan_args(plan, elem_off, fmt, stride, buf.nbytes)
        out = np.zeros(plan.total_samples, dtype=np.int16)
        self._check(L.ctu_engine_run_signal_wire_host(self._h, plan._h, buf.ctypes.data, off.ctypes.data, ctypes.byref(w), out.ctypes.data))
        n = L.ctu_plan_out_samples(plan._h)
        res = [out[plan.sample_off[i]:plan.sample_off[i] + n[i]].copy() for i in range(plan.n_utt)]
        plan.close()
        return res

    def extract_interleaved(self, frames, fmt="s16", want_vad=False):
        """A [samples, channels] numpy block - a multichannel file as it lies - as one utterance per channel, in channel order: the
        offline twin of Streams.push_interleaved (extract_wire with stride = channels, elem_off = the channel)."""
        frames = np.asarray(frames)
        assert frames.ndim == 2 and frames.flags["C_CONTIGUOUS"]
        samples, channels = frames.shape
        return self.extract_wire(frames, np.arange(channels, dtype=np.int64), np.full(channels, samples, dtype=np.int64), fmt=fmt, stride=channels,
                                 want_vad=want_vad)

    # ---- feature files in (-format_in htk)
    def run_rows_device(self, plan, words, rows=None, stream=None):
        """words: torch int32 CUDA tensor [plan.total_samples] (the files' payloads at plan.sample_off); returns the rows tensor (async)."""
        import torch
        assert words.is_cuda and words.dtype == torch.int32 and words.numel() >= plan.total_samples
        if rows is None:
            rows = torch.empty((plan.total_frames, self.dims.row_floats), dtype=torch.float32, device=words.device)
        s = stream if stream is not None else torch.cuda.current_stream(words.device)
        self._check(load_library().ctu_engine_run_rows(self._h, plan._h, words.data_ptr(), rows.data_ptr(), s.cuda_stream))
        return rows

    def run_rows_host(self, plan, arena, rows_out=None):
        """numpy uint32 arena (the files' payloads as they stand, at plan.sample_off) in, numpy float32 rows out."""
        assert arena.dtype == np.uint32 and arena.flags.c_contiguous and arena.size >= plan.total_samples
        rows = rows_out if rows_out is not None else np.empty((plan.total_frames, self.dims.row_floats), dtype=np.float32)
        self._check(load_library().ctu_engine_run_rows_host(self._h, plan._h, arena.ctypes.data, rows.ctypes.data))
        return rows

    def postprocess(self, features):
        """list of [rows, -nfeacoefs] float32 arrays (the rows of HTK feature files, in file order) -> list of [rows, D] float32 arrays:
        delta / stacking and CMS as the engine's command line says (an engine created with -format_in htk)."""
        width = self.dims.row_floats_in
        feats = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, width) for f in features]
        plan = self.plan([f.shape[0] for f in feats])
        arena = np.zeros(max(plan.total_samples, 1), dtype=np.uint32)
        order = ">u4" if self.dims.swap_in else "<u4"   # the engine reads the words in the byte order -endian_in names
        for f, off in zip(feats, plan.sample_off[:-1]):
            arena[off:off + f.size] = f.reshape(-1).view(np.uint32).astype(order).view(np.uint32)
        rows = self.run_rows_host(plan, arena)
        out = [rows[plan.row_off[i]:plan.row_off[i + 1]] for i in range(plan.n_utt)]
        plan.close()
        return out

    # ---- per-speaker CMVN over device-resident rows (include/ctu_engine.h; src/fea/post_impl.cc:51-118)
    def cmvn_cols(self):
        return int(load_library().ctu_cmvn_cols(self._h))

    def cmvn_accumulate(self, plan, rows, spk_of_utt, n_spk, mean=None, acc=None, stream=None):
        """acc[n_spk, cols+1] (float64) += sums (mean is None) or sums of squared deviations from `mean`, and counts."""
        import torch
        cols = self.cmvn_cols()
        spk = np.ascontiguousarray(spk_of_utt, dtype=np.int32)
        if acc is None:
            acc = np.zeros((n_spk, cols + 1), dtype=np.float64)
        assert acc.shape == (n_spk, cols + 1) and acc.dtype == np.float64 and acc.flags.c_contiguous
        m = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
        s = stream if stream is not None else torch.cuda.current_stream(rows.device)
        self._check(load_library().ctu_cmvn_accumulate(self._h, plan._h, rows.data_ptr(), spk.ctypes.data, int(n_spk),
                                                       m.ctypes.data if m is not None else None, acc.ctypes.data, s.cuda_stream))
        return acc

    def cmvn_apply(self, plan, rows, spk_of_utt, n_spk, mean, var, stream=None):
        import torch
        spk = np.ascontiguousarray(spk_of_utt, dtype=np.int32)
        m = np.ascontiguousarray(mean, dtype=np.float64)
        v = np.ascontiguousarray(var, dtype=np.float64)
        s = stream if stream is not None else torch.cuda.current_stream(rows.device)
        self._check(load_library().ctu_cmvn_apply(self._h, plan._h, rows.data_ptr(), spk.ctypes.data, int(n_spk),
                                                  m.ctypes.data, v.ctypes.data, s.cuda_stream))
        return rows

    def decode_g711(self, codes, alaw=True, stream=None):
        """torch uint8 CUDA tensor of G.711 codes -> int16 CUDA tensor (the reference's expansion, on the device)."""
        import torch
        assert codes.is_cuda and codes.dtype == torch.uint8
        out = torch.empty(codes.numel(), dtype=torch.int16, device=codes.device)
        s = stream if stream is not None else torch.cuda.current_stream(codes.device)
        self._check(load_library().ctu_decode_g711(self._h, codes.data_ptr(), codes.numel(), 1 if alaw else 0, out.data_ptr(), s.cuda_stream))
        return out

    def set_vad_stream(self, data):
        """-vad file=...: replaces the byte stream the hwss / fwss / 2fwss decisions are read from (one byte per frame) and rewinds it."""
        data = bytes(data)
        self._check(load_library().ctu_engine_set_vad_stream(self._h, data, len(data)))

    def reset_chain(self):
        """hwss / fwss / 2fwss: forget the spectrum vector the previous run left behind (see include/ctu_engine.h)."""
        self._check(load_library().ctu_engine_reset_chain(self._h))

    def last_kernel_ms(self):
        return float(load_library().ctu_engine_last_kernel_ms(self._h))

    def kernel_name(self):
        return load_library().ctu_engine_kernel_name(self._h).decode()

    def phase2_walk(self):
        """Index of the straight-line filter-bank walk that the last run's front end was launched with, or -1 (generic walk)."""
        return int(load_library().ctu_engine_phase2_walk(self._h))

    def vad_ring_of_list(self, nsamples, order):
        """historyIdx each file of a list starts with when the list is one process's (ctu_vad_ring_step from 0, 0)."""
        L = load_library()
        hi, hs = ctypes.c_int32(0), ctypes.c_int32(0)
        out = []
        for k, n in enumerate(nsamples):
            if hs.value != 0:   # as bin/ctucopy does (host/main.cc, half_drained): not reproduced, and not passed over in silence
                raise CtuError(CTU_ERR_UNSUPPORTED, f"VAD: file {k - 1} of the list has no more frames than the majority filter delays (-vad_filter_order {order}): "
                               "the reference's filter stays half drained for the files behind it (src/vad/vad.h:156-175), which is not reproduced")
            out.append(hi.value)
            L.ctu_vad_ring_step(int(order), max(self.num_frames(int(n)), 0), ctypes.byref(hi), ctypes.byref(hs))
        return out

    def extract(self, utterances, want_vad=False, as_list_of_one_process=None):
        """Convenience: list of int16 arrays -> list of [rows, D] float32 arrays (and the VAD byte strings).

        as_list_of_one_process = the VAD's filter order: the utterances are the files of one list, the majority filter's ring index runs
        on from file to file as in the reference (Plan.set_vad_ring)."""
        plan = self.plan([len(u) for u in utterances])
        if as_list_of_one_process:
            plan.set_vad_ring(self.vad_ring_of_list([len(u) for u in utterances], as_list_of_one_process))
        rows, vad, per = self.run_host(plan, plan.pack(utterances), want_vad=True)
        out = [rows[plan.row_off[i]:plan.row_off[i] + per[i]] for i in range(plan.n_utt)]
        vads = [vad[plan.row_off[i]:plan.row_off[i + 1]] for i in range(plan.n_utt)]
        vads = [v[v != 0] for v in vads]  # NUL = nothing written (an utterance the majority filter never got ready on)
        plan.close()
        return (out, vads) if want_vad else out
