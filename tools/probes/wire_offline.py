"""Offline wire input, what it costs: one process, C1 at 16 kHz.

(a) wire_unpack_kernel's span (HIP events around Engine.unpack_wire_device: the upload of the element offsets and the one launch) per
    format and stride 1, 2, 8, beside the front end's span on the same plan (Engine.last_kernel_ms), for a ragged batch of --utts
    utterances of 2 .. 6 s and for one file of --long-minutes minutes.  Strided layouts are [sample][channel] blocks of `stride`
    channels of which the plan's utterances are channel 0.  Recorded, not gated: the parent has no such kernel.
(b) the host path on an a-law batch from page-locked buffers: Engine.run_wire_host on the codes against the parent's way to the same
    rows - the host loop over g711 codes (wire_expand, which is decode_into's loop) into a page-locked arena, then Engine.run_host -
    interleaved, --runs times each.  Gate: the new path's median is not above the parent's by more than the parent's own spread.

    python tools/probes/wire_offline.py [--out profiles/wire_offline_times.txt] [--utts 2000] [--long-minutes 10] [--runs 7] [--reps 10]
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
from tests.util import C1  # noqa: E402

FORMATS = ("s16", "s16_swapped", "alaw", "mulaw")


def med(v):
    return "%.4f (%.4f..%.4f)" % (statistics.median(v), min(v), max(v))


def lengths(n_utt, seed=1):
    return np.random.default_rng(seed).integers(2 * 16000, 6 * 16000, n_utt).astype(np.int64)


def spans(eng, ns, fmt, stride, reps):
    """(unpack span, front-end span) in ms over `reps` runs: utterance i is the elements off[i] + k * stride of one device buffer of
    random elements (the spans do not depend on what the samples are)."""
    import torch
    plan = eng.plan(ns)
    off = np.zeros(len(ns), np.int64)
    off[1:] = np.cumsum(((ns[:-1] + 15) // 16 * 16) * stride)
    total = int(off[-1] + ns[-1] * stride)
    g711 = fmt in ("alaw", "mulaw")
    buf = (torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda") if g711
           else torch.randint(-32768, 32768, (total,), dtype=torch.int16, device="cuda"))
    pcm = torch.zeros(plan.total_samples, dtype=torch.int16, device="cuda")
    rows = torch.empty((plan.total_frames, eng.dims.row_floats), dtype=torch.float32, device="cuda")
    un, fe = [], []
    for k in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.unpack_wire_device(plan, buf, off, fmt=fmt, stride=stride, pcm=pcm)
        e1.record()
        eng.run_device(plan, pcm, rows=rows)
        torch.cuda.synchronize()
        if k >= 2:
            un.append(e0.elapsed_time(e1))
            fe.append(eng.last_kernel_ms())
    plan.close()
    return med(un), med(fe), total * (1 if g711 else 2), int(ns.sum())


def host_ab(eng, ns, runs, say):
    """(b): wall ms of the parent's way and of run_wire_host, interleaved."""
    plan = eng.plan(ns)
    off = np.zeros(len(ns), np.int64)
    off[1:] = np.cumsum((ns[:-1] + 15) // 16 * 16)
    total = int(off[-1] + ns[-1])
    codes = ceng.host_alloc((total,), np.uint8)
    codes[...] = np.random.default_rng(2).integers(0, 256, total, dtype=np.uint8)   # (the times do not depend on what the codes are)
    arena = ceng.host_alloc((plan.total_samples,), np.int16)
    rows_a = ceng.host_alloc((plan.total_frames, eng.dims.row_floats), np.float32)
    rows_b = ceng.host_alloc((plan.total_frames, eng.dims.row_floats), np.float32)
    L = ceng.load_library()
    w = ceng.WireLayout(ceng.WIRE_FORMATS["alaw"], 1)
    so = plan.sample_off
    old, new = [], []
    for k in range(runs + 1):
        t0 = time.perf_counter()
        for i in range(plan.n_utt):   # decode_into's loop, file after file, into the page-locked arena (one thread here)
            L.ctu_wire_expand(w, codes.ctypes.data, int(off[i]), int(ns[i]), arena.ctypes.data + 2 * int(so[i]))
        t1 = time.perf_counter()
        eng.run_host(plan, arena, rows_out=rows_a)
        t2 = time.perf_counter()
        eng.run_wire_host(plan, codes, off, fmt="alaw", rows_out=rows_b)
        t3 = time.perf_counter()
        assert np.array_equal(rows_a.view(np.int32), rows_b.view(np.int32)), "the two paths give other rows"
        if k >= 1:
            old.append(1e3 * (t2 - t0))
            new.append(1e3 * (t3 - t2))
            say("host_ab run %d  expand_ms %.2f  run_host_ms %.2f  parent_way_ms %.2f  run_wire_host_ms %.2f" %
                (k, 1e3 * (t1 - t0), 1e3 * (t2 - t1), old[-1], new[-1]))
    spread = max(old) - min(old)
    ok = statistics.median(new) <= statistics.median(old) + spread
    say("host_ab  utterances %d  wire_bytes %d  frames %d  parent_way_ms %s  run_wire_host_ms %s  parent_spread_ms %.2f  gate %s" %
        (plan.n_utt, total, plan.total_frames, med(old), med(new), spread, "PASS" if ok else "FAIL"))
    # run_host alone (the upload of the samples, no host loop): what the link and the kernels leave of the difference
    only = []
    for k in range(runs):
        t0 = time.perf_counter()
        eng.run_host(plan, arena, rows_out=rows_a)
        only.append(1e3 * (time.perf_counter() - t0))
    say("host_ab  run_host_alone_ms %s" % med(only))
    plan.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--long-minutes", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch  # noqa: F401  (ahead of the engine library: both then share torch's HIP runtime)
    assert torch.cuda.is_available()
    out = open(a.out, "a") if a.out else None

    def say(line):
        sys.stdout.write(line + "\n")
        sys.stdout.flush()
        if out:
            out.write(line + "\n")
            out.flush()

    eng = Engine(C1)
    say("# tools/probes/wire_offline.py: C1 at 16 kHz, %s; medians (smallest..largest) of %d runs, spans in ms from HIP events" % (eng.kernel_name(), a.reps))
    say("# (a) shape  format  stride  unpack_ms  frontend_ms  wire_bytes  samples")
    shapes = (("batch_%d" % a.utts, lengths(a.utts)), ("one_file_%gmin" % a.long_minutes, np.array([int(a.long_minutes * 60 * 16000)], np.int64)))
    for name, ns in shapes:
        for fmt in FORMATS:
            for stride in (1, 2, 8):
                say("%s  %s  %d  %s  %s  %d  %d" % ((name, fmt, stride) + spans(eng, ns, fmt, stride, a.reps)))
    say("# (b) a-law batch from page-locked buffers: the parent's way (host loop + run_host) against run_wire_host, wall ms")
    ok = host_ab(eng, lengths(a.utts), a.runs, say)
    if out:
        out.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
