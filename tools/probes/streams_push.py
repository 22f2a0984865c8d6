"""Streaming input, coverage figures: what a push costs beside the front end it feeds.

MFCC-13 at 16 kHz, pushes of 10 hops to each of N concurrent streams (N = 1 000 and 10 000), device-resident samples and rows.
Per N: the three spans of a push from HIP events on its stream (stream_stitch_kernel | front end | stream_carry_kernel, median
of the timed pushes), the push rate in frames/s from the host's clock around synchronised pushes, and the rate of one offline
device-resident run over the same frames (N utterances of 10 frames; the offline path is the parent commit's).
With --row-state the same again for MFCC_0_D_A with a running mean (-fea_delta d_a -fea_Z_exp 500) on a set with row state, in the
same run: its front-end span includes the streamed delta and CMS kernels, its carry span the base-row history.
With --nr-state the same again for C4 without its VAD (MFCC-13 at 8 kHz behind -nr_mode exten -nr_a 2) on a set with noise state: its
front end walks chains of whole streams, a wave each, and loads and stores the noise estimate at the edges of the push; the offline run
beside it is ten-frame files, each of which starts from the initial estimate.
With --vad-state the same again for C4 itself (exten and the fused Burg-cepstral VAD, adapt threshold) on a set with noise and detector
state: its front-end span has the fused detector's lattices, vad_a2c_kernel, the replay from the detector's state and the delayed
row copy in it, its carry span the history of the held rows; decisions are delivered with the rows.
With --ss-state the set with noise state again (the yardstick of the same run), then -nr_mode fwss -vad burg at 8 kHz and at 16 kHz on
sets with subtraction state: the front end runs phase 1 twice per step and the Burg lattices of the detector, and loads and stores both
noise estimates and the detector's record at the edges of the push.  What is measured is what such a push costs against the exten
set's push in the same process; the offline run beside it is one list of ten-frame files, seed iteration and its read-backs included.

    python tools/probes/streams_push.py [--out profiles/streams_push_times.txt] [--pushes 8] [--warmup 3] [--row-state] [--nr-state] [--vad-state] [--ss-state]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ctucopy_amd import Engine  # noqa: E402
from tests.util import C2, C4, C4_NOVAD, synth_utt  # noqa: E402


CHAIN = ["-fea_delta", "d_a", "-fea_Z_exp", "500"]
FWSS_8K = "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97 -vad burg -nr_mode fwss".split()
FWSS_16K = C2 + ["-vad", "burg", "-nr_mode", "fwss"]


def measure(n, pushes, warmup, chain=False, nr=False, vad=False, ss=None):
    import torch
    eng = Engine(ss if ss else C4 if vad else C4_NOVAD if nr else C2 + (CHAIN if chain else []))
    w, s, D = eng.dims.window, eng.dims.wshift, eng.dims.row_floats
    hop = 10 * s
    total = w - s + hop * (warmup + pushes)
    x = synth_utt(1, total, fs=eng.dims.fs)
    pcm = torch.from_numpy(np.tile(x, n)).cuda()
    ids = np.arange(n, dtype=np.int32)
    base = np.arange(n, dtype=np.int64) * total
    st = eng.streams(n, hop, row_state=chain, nr_state=nr or vad, vad_state=vad, ss_state=bool(ss))
    rows = torch.empty((n * 11, D), dtype=torch.float32, device="cuda")
    dec = torch.empty(n * 11, dtype=torch.uint8, device="cuda") if vad else None
    cnt = st.push_device(ids, pcm, base, np.full(n, w - s), rows, vad=dec)   # the samples ahead of the first hop: no frame yet
    assert int(cnt.sum()) == 0
    spans, wall = [], []
    for k in range(warmup + pushes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cnt = st.push_device(ids, pcm, base + (w - s) + k * hop, np.full(n, hop), rows, vad=dec)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        # (the first ten frames of a d_a file give six rows, of a file behind the VAD's majority filter of order 3 nine)
        assert int(cnt.min()) == int(cnt.max()) == ((6 if chain else 9 if vad else 10) if k == 0 else 10)
        if k >= warmup:
            spans.append(st.last_push_ms())
            wall.append(t1 - t0)
    med = [statistics.median(v[i] for v in spans) for i in range(3)]
    push_rate = 10 * n / statistics.median(wall)
    # the same frames offline: N utterances of ten frames, device-resident
    utts = [x[:w + 9 * s]] * n
    plan = eng.plan([len(u) for u in utts])
    arena = torch.from_numpy(plan.pack(utts)).cuda()
    out = torch.empty((plan.total_frames, D), dtype=torch.float32, device="cuda")
    out_vad = torch.empty(max(plan.total_frames, 1), dtype=torch.uint8, device="cuda") if vad else None
    off_wall, off_kernel = [], []
    for k in range(warmup + pushes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run_device(plan, arena, rows=out, vad=out_vad)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            off_wall.append(t1 - t0)
            off_kernel.append(eng.last_kernel_ms())
    assert plan.total_frames == 10 * n
    return med, push_rate, statistics.median(off_kernel), 10 * n / statistics.median(off_wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pushes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--row-state", action="store_true", help="also MFCC_0_D_A with exponential CMS on a set with row state")
    ap.add_argument("--nr-state", action="store_true", help="also C4 without its VAD (-nr_mode exten) on a set with noise state")
    ap.add_argument("--vad-state", action="store_true", help="also C4 (exten and the fused Burg-cepstral VAD) on a set with noise and detector state")
    ap.add_argument("--ss-state", action="store_true", help="also the exten set again, then -nr_mode fwss -vad burg at 8 and 16 kHz on sets with subtraction state")
    a = ap.parse_args()
    lines = ["# tools/probes/streams_push.py: MFCC-13, 16 kHz, pushes of 10 hops per stream, device-resident; medians of %d pushes after %d" % (a.pushes, a.warmup),
             "# spans from HIP events on the push's stream; rates from the host's clock around synchronised calls (launch overhead included)",
             "# streams  stitch_ms  frontend_ms  carry_ms  push_frames_per_s  offline_frontend_ms  offline_frames_per_s"]
    ss_runs = [(False, True, False, None), (False, False, False, FWSS_8K), (False, False, False, FWSS_16K)] if a.ss_state else []
    for chain, nr, vad, ss in [(False, False, False, None)] + ([(True, False, False, None)] if a.row_state else []) + ([(False, True, False, None)] if a.nr_state else []) + \
            ([(False, False, True, None)] if a.vad_state else []) + ss_runs:
        if ss:
            lines.append("# " + " ".join(ss) + " on a set with subtraction state (frontend_ms: chains of whole streams, a wave each, phase 1 twice per step and the"
                         " detector's Burg lattices, both noise estimates and the detector's record loaded and stored at the edges of the push; the offline run is"
                         " one list of ten-frame files: offline_frontend_ms spans the seed iteration with its read-backs)")
        if vad:
            lines.append("# " + " ".join(C4) + " on a set with noise and detector state (frontend_ms: with the fused detector, vad_a2c_kernel, the replay"
                         " from the detector's state and the delayed row copy; carry_ms: with the history of the held rows; the offline run is files of ten"
                         " frames with vad_lanes_kernel behind the front end, outside offline_frontend_ms)")
        if nr:
            lines.append("# " + " ".join(C4_NOVAD) + " on a set with noise state (frontend_ms: chains of whole streams, a wave each, the noise estimate loaded"
                         " and stored at the edges of the push; the offline run is files of ten frames, each from the initial estimate)")
        if chain:
            lines.append("# the same with " + " ".join(CHAIN) + " on a set with row state (frontend_ms: with the streamed delta and CMS kernels; carry_ms: with"
                         " the base-row history; offline_frontend_ms is the front end alone, the offline rate has post_kernel and cms_exp_kernel in it)")
        for n in (1000, 10000):
            med, pr, ok, orate = measure(n, a.pushes, a.warmup, chain, nr, vad, ss)
            lines.append("%7d  %.4f  %.4f  %.4f  %.3e  %.4f  %.3e" % (n, med[0], med[1], med[2], pr, ok, orate))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
