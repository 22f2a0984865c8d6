"""Stream sets with large-transform state, coverage figures (Large-transform state): what one push costs.

2048-point frames (44.1 kHz, 25 ms), -nr_mode exten: one push of 8 frames to each of 64 streams, on the feature path (noise state) and
with speech output (noise and signal state).  The three spans of the push from HIP events on its stream (ctu_streams_last_push_ms:
stream_stitch_kernel | the kernels of the run, with the synthesis and the overlap-add for speech | stream_carry_kernel; median of the
timed pushes), and beside them the offline run of the same 512 frames as 64 files of 8 (ctu_engine_last_kernel_ms: bigfft_kernel's
span; those kernels are not changed by the stream sets).

    python tools/probes/streams_large_push.py [--out profiles/streams_large_push_times.txt] [--pushes 8] [--warmup 3]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ctucopy_amd import Engine  # noqa: E402
from tests.util import synth_utt  # noqa: E402

FEATURES = "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97 -nr_mode exten".split()
SPEECH = "-fs 44100 -format_in raw -format_out raw -w 24 -s 12.5 -nr_mode exten".split()
N, FRAMES = 64, 8


def measure(cfg, pushes, warmup):
    eng = Engine(cfg)
    speech = eng.dims.signal_out == 1
    w, s = eng.dims.window, eng.dims.wshift
    hop = FRAMES * s
    x = synth_utt(1, w - s + hop * (warmup + pushes), fs=eng.dims.fs)
    st = eng.streams(N, max(hop, w - s), nr_state=True, signal_state=speech, large_state=True)
    push = st.push_signal if speech else st.push
    push({i: x[:w - s] for i in range(N)})   # the samples ahead of the first hop: no frame yet
    spans = []
    for k in range(warmup + pushes):
        at = w - s + k * hop
        out = push({i: x[at:at + hop] for i in range(N)})
        assert all((v.size if speech else v.shape[0]) == (hop if speech else FRAMES) for v in out.values())
        if k >= warmup:
            spans.append(st.last_push_ms())
    med = [statistics.median(v[i] for v in spans) for i in range(3)]
    utts = [x[:w + (FRAMES - 1) * s]] * N
    off = []
    for k in range(warmup + pushes):
        (eng.enhance if speech else eng.extract)(utts)
        if k >= warmup:
            off.append(eng.last_kernel_ms())
    return eng.kernel_name(), med, statistics.median(off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    lines = ["# tools/probes/streams_large_push.py: one push of %d frames to each of %d streams at 2048 points behind -nr_mode exten, on a set with" % (FRAMES, N),
             "# noise and large-transform state (features) and with signal state as well (speech); medians of %d pushes after %d." % (a.pushes, a.warmup),
             "# Spans from HIP events on the push's stream (ctu_streams_last_push_ms; run_ms: bigfft_kernel<8, true, XS> and, for speech,",
             "# bigsynth_kernel and the overlap-add).  offline_kernel_ms: ctu_engine_last_kernel_ms of the offline run over the same %d frames" % (N * FRAMES),
             "# as %d files of %d (bigfft_kernel<8, true>, a kernel the stream sets do not change; speech: without bigsynth_kernel and ola_kernel)." % (N, FRAMES),
             "# Information, not a gate: these kernels exist for coverage.",
             "# chain  kernel  stitch_ms  run_ms  carry_ms  offline_kernel_ms"]
    for name, cfg in (("features", FEATURES), ("speech", SPEECH)):
        kern, med, off = measure(cfg, a.pushes, a.warmup)
        lines.append("%s  %s  %.4f  %.4f  %.4f  %.4f" % (name, kern, med[0], med[1], med[2], off))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
