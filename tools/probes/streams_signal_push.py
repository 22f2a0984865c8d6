"""Streaming speech output, coverage figures (Signal state): what a push on a set with signal state costs.

-preset exten at 16 kHz (512-point frames, a hop of 256 samples) on a set with noise and signal state, pushes of 10 hops to each of N
concurrent streams (N = 1 000 and 10 000), device-resident samples in and out.  Per N: the three spans of a push from HIP events on its
stream (stream_stitch_kernel | front end with its synthesis and stream_ola_kernel | stream_carry_kernel, median of the timed pushes),
the rate in samples/s from the host's clock around synchronised pushes, and beside it ctu_engine_run_signal over the same frames
(N utterances of 10 frames, device-resident; that offline path is not changed by the stream sets): its front-end span and its rate.

    python tools/probes/streams_signal_push.py [--out profiles/streams_signal_push_times.txt] [--pushes 8] [--warmup 3]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ctucopy_amd import Engine  # noqa: E402
from tests.util import SIG_EXTEN, synth_utt  # noqa: E402


def measure(n, pushes, warmup):
    import torch
    eng = Engine(SIG_EXTEN)
    w, s = eng.dims.window, eng.dims.wshift
    hop = 10 * s
    total = w - s + hop * (warmup + pushes)
    x = synth_utt(1, total, fs=eng.dims.fs)
    pcm = torch.from_numpy(np.tile(x, n)).cuda()
    ids = np.arange(n, dtype=np.int32)
    base = np.arange(n, dtype=np.int64) * total
    st = eng.streams(n, hop, nr_state=True, signal_state=True)
    out = torch.empty(n * hop, dtype=torch.int16, device="cuda")
    cnt = st.push_signal_device(ids, pcm, base, np.full(n, w - s), out)   # the samples ahead of the first hop: no frame yet
    assert int(cnt.sum()) == 0
    spans, wall = [], []
    for k in range(warmup + pushes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cnt = st.push_signal_device(ids, pcm, base + (w - s) + k * hop, np.full(n, hop), out)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        assert int(cnt.min()) == int(cnt.max()) == hop
        if k >= warmup:
            spans.append(st.last_push_ms())
            wall.append(t1 - t0)
    med = [statistics.median(v[i] for v in spans) for i in range(3)]
    push_rate = hop * n / statistics.median(wall)
    # the same frames offline: N utterances of ten frames, device-resident
    utts = [x[:w + 9 * s]] * n
    plan = eng.plan([len(u) for u in utts])
    arena = torch.from_numpy(plan.pack(utts)).cuda()
    off = torch.zeros(plan.total_samples, dtype=torch.int16, device="cuda")
    off_wall, off_kernel = [], []
    for k in range(warmup + pushes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.enhance_device(plan, arena, out=off)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            off_wall.append(t1 - t0)
            off_kernel.append(eng.last_kernel_ms())
    assert plan.total_frames == 10 * n
    return med, push_rate, statistics.median(off_kernel), hop * n / statistics.median(off_wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    lines = ["# tools/probes/streams_signal_push.py: " + " ".join(SIG_EXTEN) + " on a set with noise and signal state, pushes of 10 hops per stream,",
             "# device-resident; medians of %d pushes after %d.  Spans from HIP events on the push's stream (frontend_ms: the front end with its" % (a.pushes, a.warmup),
             "# synthesis, chains of whole streams, and stream_ola_kernel); rates in delivered samples per second from the host's clock around",
             "# synchronised calls (launch overhead included).  Offline: ctu_engine_run_signal over files of ten frames (offline_frontend_ms: its front end;",
             "# the offline rate counts the same 10 hops per file and has ola_kernel, which also writes every file's tail, in it)",
             "# streams  stitch_ms  frontend_ms  carry_ms  push_samples_per_s  offline_frontend_ms  offline_samples_per_s"]
    for n in (1000, 10000):
        med, pr, ok, orate = measure(n, a.pushes, a.warmup)
        lines.append("%7d  %.4f  %.4f  %.4f  %.3e  %.4f  %.3e" % (n, med[0], med[1], med[2], pr, ok, orate))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
