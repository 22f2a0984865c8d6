"""Streaming speech output, coverage figures (Signal state): what a push on a set with signal state costs.

-preset exten at 16 kHz (512-point frames, a hop of 256 samples) on a set with noise and signal state, pushes of 10 hops to each of N
concurrent streams (N = 1 000 and 10 000), device-resident samples in and out.  Per N: the three spans of a push from HIP events on its
stream (stream_stitch_kernel | front end with its synthesis and stream_ola_kernel | stream_carry_kernel, median of the timed pushes),
the rate in samples/s from the host's clock around synchronised pushes, and beside it ctu_engine_run_signal over the same frames
(N utterances of 10 frames, device-resident; that offline path is not changed by the stream sets): its front-end span and its rate.

With --ss-state instead: -nr_mode fwss -vad burg with speech output at 8 and 16 kHz (-w 25 -s 12.5) on a set with subtraction and signal
state (CTU_STREAMS_SS_SIGNAL_STATE), the same protocol without the offline column (a list of N ten-frame files is the worst case of the offline seed iteration).

    python tools/probes/streams_signal_push.py [--ss-state] [--out profiles/streams_signal_push_times.txt] [--pushes 8] [--warmup 3]
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


def sig_fwss(fs):
    return ("-fs %d -format_in raw -format_out raw -w 25 -s 12.5 -nr_mode fwss -vad burg" % fs).split()


def measure(n, pushes, warmup, cfg=SIG_EXTEN, ss=False):
    import torch
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    hop = 10 * s
    total = w - s + hop * (warmup + pushes)
    x = synth_utt(1, total, fs=eng.dims.fs)
    pcm = torch.from_numpy(np.tile(x, n)).cuda()
    ids = np.arange(n, dtype=np.int32)
    base = np.arange(n, dtype=np.int64) * total
    st = eng.streams(n, hop, signal_state=True, ss_state=True, ss_signal_state=True) if ss else eng.streams(n, hop, nr_state=True, signal_state=True)
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
    if ss:  # (no offline column: a list of N ten-frame files is the seed iteration's worst case, seconds per run - DESIGN.md section 4.10)
        return med, push_rate, None, None
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
    ap.add_argument("--ss-state", action="store_true", help="fwss at 8 and 16 kHz on a set with subtraction and signal state")
    a = ap.parse_args()
    if a.ss_state:
        return main_ss(a)
    lines = ["# tools/probes/streams_signal_push.py: " + " ".join(SIG_EXTEN) + " on a set with noise and signal state, pushes of 10 hops per stream,",
             "# device-resident; medians of %d pushes after %d.  Spans from HIP events on the push's stream (frontend_ms: the front end with its" % (a.pushes, a.warmup),
             "# synthesis, chains of whole streams, and stream_ola_kernel); rates in delivered samples per second from the host's clock around",
             "# synchronised calls (launch overhead included).  Offline: ctu_engine_run_signal over files of ten frames (offline_frontend_ms: its front end;",
             "# the offline rate counts the same 10 hops per file and has ola_kernel, which also writes every file's tail, in it)",
             "# streams  stitch_ms  frontend_ms  carry_ms  push_samples_per_s  offline_frontend_ms  offline_samples_per_s"]
    for n in (1000, 10000):
        med, pr, ok, orate = measure(n, a.pushes, a.warmup)
        lines.append("%7d  %.4f  %.4f  %.4f  %.3e  %.4f  %.3e" % (n, med[0], med[1], med[2], pr, ok, orate))
    write(lines, a.out)


def main_ss(a):
    lines = ["# tools/probes/streams_signal_push.py --ss-state: -w 25 -s 12.5 -nr_mode fwss -vad burg with speech output on a set with subtraction and",
             "# signal state, pushes of 10 hops per stream, device-resident; medians of %d pushes after %d, the columns of the exten rows." % (a.pushes, a.warmup),
             "# (no offline column: a list of N ten-frame files is the worst case of the offline seed iteration and takes seconds per run)",
             "# fs  streams  stitch_ms  frontend_ms  carry_ms  push_samples_per_s"]
    for fs in (8000, 16000):
        for n in (1000, 10000):
            med, pr, _, _ = measure(n, a.pushes, a.warmup, sig_fwss(fs), True)
            lines.append("%5d  %7d  %.4f  %.4f  %.4f  %.3e" % (fs, n, med[0], med[1], med[2], pr))
    write(lines, a.out)


def write(lines, out):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
