"""Wire input, what a push costs ("Wire input"): one process, C1 at 8 kHz, 1 024 streams, pushes of 80, 160 and
1 600 samples per stream.

(a) the plain path: the spans of Streams.push_device (stream_stitch_kernel | front end | stream_carry_kernel, HIP events) on contiguous
    native samples.  Run once per library (CTU_ENGINE_LIB names another build of it: the yardstick of an A/B; a library without the
    wire calls runs (a) alone).
(b) the wire path: the same samples through push_wire_device in each format, contiguous and interleaved as one [samples, 1024] block:
    stream_stitch_wire_kernel's span beside the front end's.
(c) the host forms: wall time of Streams.push with its 1 024 pointers against push_wire on one contiguous and on one interleaved
    block, a-law and S16, from pageable and from page-locked buffers.

Every figure is the median of --pushes timed pushes after --warmup untimed ones, with their smallest .. largest value beside it; the
whole probe is run --runs times in one process and the figures of every run are printed.

    python tools/probes/streams_wire_push.py [--out profiles/streams_wire_push_times.txt] [--pushes 20] [--warmup 5] [--runs 3] [--tag tree]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ctucopy_amd import Engine  # noqa: E402
from ctucopy_amd import engine as ceng  # noqa: E402
from tests.util import C1, ref_outputs, synth_utt  # noqa: E402

N = 1024
SIZES = (80, 160, 1600)
C1_8K = ["-fs", "8000"] + C1[2:]


def med(v):
    return "%.4f (%.4f..%.4f)" % (statistics.median(v), min(v), max(v))


def raw_of(fmt, x):
    if fmt == "s16":
        return x
    if fmt == "s16_swapped":
        return x.byteswap()
    t = ref_outputs()["amulaw_a" if fmt == "alaw" else "amulaw_mu"]
    order = np.argsort(t, kind="stable")
    return order[np.clip(np.searchsorted(t[order], x), 0, 255)].astype(np.uint8)


def device_spans(eng, size, pushes, warmup, fmt=None, interleaved=False):
    """Medians of the three spans over the timed pushes: plain (fmt None) or wire."""
    import torch
    w, s, D = eng.dims.window, eng.dims.wshift, eng.dims.row_floats
    total = size * (warmup + pushes)
    x = raw_of(fmt or "s16", synth_utt(1, total, fs=eng.dims.fs))
    ids = np.arange(N, dtype=np.int32)
    ns = np.full(N, size, dtype=np.int64)
    st = eng.streams(N, size)
    rows = torch.empty((N * (size // s + 2), D), dtype=torch.float32, device="cuda")
    if interleaved:
        buf = torch.from_numpy(np.ascontiguousarray(np.tile(x[:, None], (1, N)))).cuda()   # [total, N]: one block, every push a range of rows
    else:
        buf = torch.from_numpy(np.tile(x, N)).cuda()                                          # stream i at i * total
    spans = []
    for k in range(warmup + pushes):
        if interleaved:
            off = (np.arange(N, dtype=np.int64) + k * size * N)
            st.push_wire_device(ids, buf, off, ns, rows, fmt=fmt, stride=N)
        elif fmt is None:
            st.push_device(ids, buf, np.arange(N, dtype=np.int64) * total + k * size, ns, rows)
        else:
            st.push_wire_device(ids, buf, np.arange(N, dtype=np.int64) * total + k * size, ns, rows, fmt=fmt)
        if k >= warmup:
            spans.append(st.last_push_ms())
    torch.cuda.synchronize()
    st.close()
    return [med([v[i] for v in spans]) for i in range(3)]


def host_wall(eng, size, pushes, warmup, how, fmt="s16", pinned=False):
    """Median wall time in ms of a synchronised host push: how = "pointers" (Streams.push), "contiguous" or "interleaved" (push_wire)."""
    total = size * (warmup + pushes)
    x = raw_of(fmt, synth_utt(1, total, fs=eng.dims.fs))
    ids = np.arange(N, dtype=np.int32)
    ns = np.full(N, size, dtype=np.int64)
    st = eng.streams(N, size)
    if how == "pointers":
        per = [x.copy() for _ in range(N)]
    else:
        # interleaved: [total, N], a push is a range of rows; contiguous: [push][stream][size], a push is one of the outer blocks -
        # either way the covering range of a push is the N * size elements a set stages
        block = (np.ascontiguousarray(np.tile(x[:, None], (1, N))) if how == "interleaved"
                 else np.ascontiguousarray(np.tile(x.reshape(-1, 1, size), (1, N, 1))).reshape(-1))
        if pinned:
            h = ceng.host_alloc(block.shape, block.dtype)
            h[...] = block
            block = h
    wall = []
    for k in range(warmup + pushes):
        t0 = time.perf_counter()
        if how == "pointers":
            st.push({i: per[i][k * size:(k + 1) * size] for i in range(N)})
        elif how == "interleaved":
            st.push_wire(block, ids, np.arange(N, dtype=np.int64) + k * size * N, ns, fmt=fmt, stride=N)
        else:
            st.push_wire(block, ids, (np.arange(N, dtype=np.int64) + k * N) * size, ns, fmt=fmt)
        t1 = time.perf_counter()
        if k >= warmup:
            wall.append(1e3 * (t1 - t0))
    st.close()
    return med(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--pushes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tag", default="tree")
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (ahead of the engine library: both then share torch's HIP runtime)
    assert torch.cuda.is_available()
    out = open(a.out, "a") if a.out else None

    class Lines:
        def append(self, line):
            sys.stdout.write(line + "\n")
            sys.stdout.flush()
            if out:
                out.write(line + "\n")
                out.flush()
    lines = Lines()
    for line in ["# tools/probes/streams_wire_push.py: C1 at 8 kHz, %d streams; medians of %d pushes after %d (smallest..largest); spans in ms from HIP events"
             % (N, a.pushes, a.warmup), "# library  run  what  samples_per_stream  stitch_ms  frontend_ms  carry_ms"]:
        lines.append(line)
    eng = Engine(C1_8K)
    wire = hasattr(ceng.load_library(), "ctu_streams_push_wire") and not a.plain_only
    for run in range(a.runs):
        for size in SIZES:
            lines.append("%s %d plain %d  %s" % (a.tag, run, size, "  ".join(device_spans(eng, size, a.pushes, a.warmup))))
        if not wire:
            continue
        for fmt in ("s16", "s16_swapped", "alaw", "mulaw"):
            for inter in (False, True):
                for size in SIZES:
                    lines.append("%s %d wire:%s:%s %d  %s" % (a.tag, run, fmt, "interleaved" if inter else "contiguous", size,
                                                              "  ".join(device_spans(eng, size, a.pushes, a.warmup, fmt, inter))))
    if wire:
        lines.append("# host forms: wall ms of one synchronised call (binding included)")
        lines.append("# library  run  what  samples_per_stream  wall_ms")
        for run in range(a.runs):
            for size in SIZES:
                lines.append("%s %d host:pointers:s16 %d  %s" % (a.tag, run, size, host_wall(eng, size, a.pushes, a.warmup, "pointers")))
                for fmt in ("s16", "alaw"):
                    for how in ("contiguous", "interleaved"):
                        for pinned in (False, True):
                            lines.append("%s %d host:%s:%s:%s %d  %s" % (a.tag, run, how, fmt, "page-locked" if pinned else "pageable", size,
                                                                         host_wall(eng, size, a.pushes, a.warmup, how, fmt, pinned)))
    if out:
        out.close()


if __name__ == "__main__":
    main()
