"""Stream sets with trap state, what one push costs (Trap state).

C5 (-preset mfcc -fb_definition 23filters -fea_kind trapdct,101,16) on a set of 1024 streams with CTU_STREAMS_TRAP_STATE, every stream
past its first 51 frames: pushes of `--hops` frames to each stream (1, 4 and 16 by default), so a push delivers 1024 x hops rows.
The three spans of the push from HIP events on its stream (ctu_streams_last_push_ms: stream_stitch_kernel | the front end,
stream_trap_kernel | stream_carry_kernel and stream_rows_carry_kernel; median of the timed pushes).  Beside them the offline run over
the same number of output rows, as files of 64 frames (ctu_engine_last_kernel_ms is the front end's span there; the offline TRAP
kernel's own time is in the kernel trace).

Kernel times come from a run of this script under a kernel trace, one hop count at a time so that a kernel name's mean is one shape's:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/probes/streams_trap_push.py --hops 4

    python tools/probes/streams_trap_push.py [--hops 1 4 16] [--out profiles/...] [--pushes 20] [--warmup 5]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ctucopy_amd import Engine  # noqa: E402
from tests.util import C5, synth_utt  # noqa: E402

N = 1024
HALF = 50


def measure(eng, hops, pushes, warmup):
    w, s = eng.dims.window, eng.dims.wshift
    hop = hops * s
    lead = w + HALF * s                       # 51 frames: from here on a push delivers a row per frame
    x = synth_utt(1, lead + hop * (warmup + pushes), fs=eng.dims.fs)
    st = eng.streams(N, max(hop, 17 * s), trap_state=True)
    at = 0
    while at < lead:                          # the lead in pushes the set takes
        n = min(17 * s, lead - at)
        st.push({i: x[at:at + n] for i in range(N)})
        at += n
    assert st.frames(0) == 1 and st.pending(0) == HALF
    spans, walls = [], []
    for k in range(warmup + pushes):
        t0 = time.perf_counter()
        out = st.push({i: x[at:at + hop] for i in range(N)})   # (host form: synchronised on return)
        t1 = time.perf_counter()
        at += hop
        assert all(v.shape[0] == hops for v in out.values())
        if k >= warmup:
            spans.append(st.last_push_ms())
            walls.append((t1 - t0) * 1e3)
    st.close()
    med = [statistics.median(v[i] for v in spans) for i in range(3)]
    # the offline run over as many rows: files of 64 frames
    utts = [x[:w + 63 * s]] * (N * hops // 64)
    off = []
    for k in range(warmup + pushes):
        rows = eng.extract(utts)
        if k >= warmup:
            off.append(eng.last_kernel_ms())
    assert sum(r.shape[0] for r in rows) == N * hops
    return med, statistics.median(walls), statistics.median(off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--hops", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--pushes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    eng = Engine(C5)
    lines = ["# tools/probes/streams_trap_push.py: C5 (trapdct,101,16, 23 bands) on %d streams with trap state, every stream past its first %d" % (N, HALF + 1),
             "# frames; one push of `hops` frames to each stream delivers %d x hops rows.  Medians of %d pushes after %d." % (N, a.pushes, a.warmup),
             "# Spans from HIP events on the push's stream (ctu_streams_last_push_ms): stitch_ms stream_stitch_kernel; run_ms the front end and",
             "# stream_trap_kernel (and the descriptors' uploads between them); carry_ms stream_carry_kernel and stream_rows_carry_kernel.",
             "# host_ms: the whole ctu_streams_push_host call (staging, upload, the push, the rows' download), host clock, synchronised.",
             "# offline_front_ms: ctu_engine_last_kernel_ms of the offline run over as many rows, as %d x hops / 64 files of 64 frames" % N,
             "# (the front end's span: the offline TRAP kernel's own time is in the kernel trace below).  Information, not a gate.",
             "# hops  rows  stitch_ms  run_ms  carry_ms  host_ms  offline_front_ms"]
    for hops in a.hops:
        med, wall, off = measure(eng, hops, a.pushes, a.warmup)
        lines.append("%d  %d  %.4f  %.4f  %.4f  %.3f  %.4f" % (hops, N * hops, med[0], med[1], med[2], wall, off))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
