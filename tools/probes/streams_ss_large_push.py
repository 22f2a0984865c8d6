"""Stream sets with subtraction state on large transforms, coverage figures (Subtraction state on large
transforms): what one push costs.

-nr_mode fwss -vad burg on 2048-point frames (44.1 kHz, 25 ms) and on 4096-point frames (48 kHz, -w 64 -s 20): pushes of one hop and of
eight hops to each of 64 streams of a set with subtraction state and its large-transform flag.  The three spans of the push from HIP
events on its stream (ctu_streams_last_push_ms: stream_stitch_kernel | the export, the detector, ss_decide_stream_kernel and
bigss_kernel<NIT, true> | stream_carry_kernel; median of the timed pushes), and beside them a FRESH engine's offline run of the same
number of frames as 64 files (ctu_engine_last_kernel_ms: the span of the export, the detector and the passes of the seed iteration
with their read-backs; and the wall time of extract, copies included).

    python tools/probes/streams_ss_large_push.py [--out profiles/streams_ss_large_push_times.txt] [--pushes 8] [--warmup 3]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ctucopy_amd import Engine  # noqa: E402
from tests.util import synth_utt  # noqa: E402

CONFIGS = (("2048", "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97 -vad burg -nr_mode fwss".split()),
           ("4096", "-fs 48000 -format_in raw -format_out htk -preset mfcc -preem 0.97 -w 64 -s 20 -vad burg -nr_mode fwss".split()))
N = 64


def measure(cfg, frames, pushes, warmup):
    eng = Engine(cfg)
    w, s = eng.dims.window, eng.dims.wshift
    hop = frames * s
    x = synth_utt(1, w - s + hop * (warmup + pushes), fs=eng.dims.fs)
    st = eng.streams(N, max(hop, w - s), ss_state=True, ss_large_state=True)
    st.push({i: x[:w - s] for i in range(N)})   # the samples ahead of the first hop: no frame yet
    spans = []
    for k in range(warmup + pushes):
        at = w - s + k * hop
        out = st.push({i: x[at:at + hop] for i in range(N)})
        assert all(v.shape[0] == frames for v in out.values())
        if k >= warmup:
            spans.append(st.last_push_ms())
    med = [statistics.median(v[i] for v in spans) for i in range(3)]
    utts = [x[:w + (frames - 1) * s]] * N
    kern, wall = [], []
    for k in range(warmup + pushes):
        fresh = Engine(cfg)   # an engine keeps its last file's vector from run to run: a fresh one starts every list from zero
        t0 = time.perf_counter()
        fresh.extract(utts)
        t1 = time.perf_counter()
        if k >= warmup:
            kern.append(fresh.last_kernel_ms())
            wall.append((t1 - t0) * 1e3)
        fresh.close()
    return eng.kernel_name(), med, statistics.median(kern), statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    lines = ["# tools/probes/streams_ss_large_push.py: one push of 1 or 8 frames to each of %d streams behind -nr_mode fwss -vad burg, on a set with" % N,
             "# subtraction state on large transforms (CTU_STREAMS_SS_STATE | CTU_STREAMS_SS_LARGE_STATE); medians of %d pushes after %d." % (a.pushes, a.warmup),
             "# Spans from HIP events on the push's stream (ctu_streams_last_push_ms; run_ms: bigfft_kernel's export, bigssdet_kernel,",
             "# ss_decide_stream_kernel, bigss_kernel<NIT, true>).  offline_kernel_ms: ctu_engine_last_kernel_ms of a fresh engine's offline run over",
             "# the same %d x frames as %d files (export, detector, ss_decide_kernel and the passes of the seed iteration with their read-backs);" % (N, N),
             "# offline_wall_ms: that extract call from the host, copies included.  Information, not a gate: these kernels exist for coverage.",
             "# points  frames_per_push  offline_kernel  stitch_ms  run_ms  carry_ms  offline_kernel_ms  offline_wall_ms"]
    for name, cfg in CONFIGS:
        for frames in (1, 8):
            kern, med, off, wall = measure(cfg, frames, a.pushes, a.warmup)
            lines.append("%s  %d  %s  %.4f  %.4f  %.4f  %.4f  %.4f" % (name, frames, kern, med[0], med[1], med[2], off, wall))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
