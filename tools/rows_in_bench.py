"""Device-resident timing of the HTK-input path: rows_ingest_kernel alone and the d_a + CMS run behind it, on
--utts files of --rows rows of 13 floats (default 6000 x 1500 = 9.0 M rows).  HIP events around `--iters` calls after `--warmup`;
achieved bytes/s from the algorithmic traffic against the 8 TB/s HBM figure of DESIGN.md.  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats` with --iters 3."""
import argparse
import json
import sys
import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctucopy_amd  # noqa: E402

HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=6000)
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    W = 13
    base = "-fs 16000 -format_in htk -format_out htk -preset mfcc -fea_rawenergy on".split()
    rng = np.random.default_rng(1)
    out = {"utts": a.utts, "rows_per_utt": a.rows, "total_rows": a.utts * a.rows}
    for name, extra, big in (("ingest", [], False), ("ingest_swap", ["-endian_in", "big"], True), ("d_a", ["-fea_delta", "d_a"], False),
                             ("d_a_cms_exp", ["-fea_delta", "d_a", "-fea_Z_exp", "500"], False)):
        e = ctucopy_amd.Engine(base + extra)
        plan = e.plan([a.rows] * a.utts)
        words = torch.from_numpy(rng.standard_normal(plan.total_samples, dtype=np.float32).view(np.int32)).cuda()
        D = e.dims.row_floats
        rows = torch.empty((plan.total_frames, D), dtype=torch.float32, device="cuda")
        for _ in range(a.warmup):
            e.run_rows_device(plan, words, rows)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kms = []
        ev0.record()
        for _ in range(a.iters):
            e.run_rows_device(plan, words, rows)
        ev1.record()
        torch.cuda.synchronize()
        for _ in range(3):  # the engine's own event pair brackets the ingest launch of the last run
            e.run_rows_device(plan, words, rows)
            kms.append(e.last_kernel_ms())
        call_ms = ev0.elapsed_time(ev1) / a.iters
        n = plan.total_frames
        ingest_bytes = 2 * 4 * W * n                                  # 4 W in + 4 W out
        run_bytes = ingest_bytes + (0 if D == W else 4 * W * n + 4 * D * n) + (0 if "cms" not in name else 2 * 4 * W * n)
        out[name] = {"call_ms": round(call_ms, 4), "ingest_kernel_ms": round(float(np.median(kms)), 4), "row_floats": D,
                     "ingest_bytes_per_s": round(ingest_bytes / (np.median(kms) * 1e-3), 1),
                     "ingest_share_of_hbm": round(ingest_bytes / (np.median(kms) * 1e-3) / HBM, 4),
                     "run_algorithmic_bytes": run_bytes, "run_bytes_per_s": round(run_bytes / (call_ms * 1e-3), 1),
                     "run_share_of_hbm": round(run_bytes / (call_ms * 1e-3) / HBM, 4), "rows_per_s": round(n / (call_ms * 1e-3), 1)}
        plan.close()
        e.close()
        del words, rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
