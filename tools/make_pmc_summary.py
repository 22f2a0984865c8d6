#!/usr/bin/env python3
"""profiles/<tag>_pmc_summary.txt and profiles/traffic.json from one profiling visit's outputs.  Run where the repository is (no GPU).

usage: tools/make_pmc_summary.py <dir> <tag> "<what build the counters were taken on>" [<dir of the build before> "<what>"]

<dir> holds what the passes of tools/final_prof.sh leave behind: pmc_summary.txt (counter, mean per dispatch of the front-end
kernel; every rocprofv3 --pmc pass a run of its own, no tracing beside it), kernel_stats.csv (rocprofv3 --kernel-trace --stats,
a run of its own) and bench_full.json (bench.py --full, unprofiled).  The kernel statistics are copied to profiles/<tag>_bench_kernel_stats.csv.  With a second
directory the summary also carries the per-frame table of the build before, side by side."""
import csv, json, shutil, sys

F = 9009528  # frames per launch of the bench workload
# Issue slots per frame at the in-situ prices (profiles/r04_frontend_cost_model.txt).  Anchor: the packed phase 1 of round 4 was
# priced at 197.0 slots when the kernel issued 123.2 vector instructions per frame.  Phase 1 has not changed since; every
# instruction that left the kernel after that left phase 2's walk and was a plain one-slot form (moves, adds, compares, selects,
# v_readfirstlane), so the slots fall by the measured fall of SQ_INSTS_VALU.  Move the anchor when phase 1 changes.
ANCHOR_VALU, ANCHOR_SLOTS = 123.2, 197.0


def read(d):
    c = {l.split()[0]: float(l.split()[1]) for l in open(d + '/pmc_summary.txt').read().rstrip('\n').split('\n')}
    rows = [r for r in csv.reader(open(d + '/kernel_stats.csv'))]
    fr = [r for r in rows[1:] if 'frontend_kernel' in r[0]][0]
    kt, calls = float(fr[3]) * 1e-9, fr[1]
    b = json.load(open(d + '/bench_full.json'))
    g = lambda k: c.get(k, float('nan'))
    v = dict(valu=g('SQ_INSTS_VALU') / F, salu=g('SQ_INSTS_SALU') / F, ldsi=g('SQ_INSTS_LDS') / F, lds=g('SQ_LDS_IDX_ACTIVE') / F,
             conf=g('SQ_LDS_BANK_CONFLICT') / F, smem=g('SQ_INSTS_SMEM') / F, vrd=g('SQ_INSTS_VMEM_RD') / F, vwr=g('SQ_INSTS_VMEM_WR') / F,
             hbm=(2 * g('FETCH_SIZE') + g('WRITE_SIZE')) * 1024 / F, wia=g('SQ_WAIT_INST_ANY') / g('SQ_WAVE_CYCLES'),
             wa=g('SQ_WAIT_ANY') / g('SQ_WAVE_CYCLES'), wil=g('SQ_WAIT_INST_LDS') / g('SQ_WAVE_CYCLES'), kt=kt * 1e3, calls=calls,
             clk=g('GRBM_GUI_ACTIVE') / 8 / kt / 1e9, ev=b['roofline']['kernel_ms'], fps=b['value'] / 1e9, kernel=b['roofline']['kernel'])
    v['slots'] = ANCHOR_SLOTS - (ANCHOR_VALU - v['valu'])
    return c, v, b


ROWS = [('HBM traffic, B (2 x FETCH_SIZE + WRITE_SIZE, KiB; algorithmic 372 B)', 'hbm', '%.0f'),
        ('VALU wave-instructions (SQ_INSTS_VALU)', 'valu', '%.1f'),
        ('  issue slots at the in-situ prices (anchor %.1f slots at %.1f instructions)' % (ANCHOR_SLOTS, ANCHOR_VALU), 'slots', '%.1f'),
        ('SALU instructions (SQ_INSTS_SALU)', 'salu', '%.1f'),
        ('LDS instructions (SQ_INSTS_LDS)', 'ldsi', '%.2f'),
        ('LDS-array cycles (SQ_LDS_IDX_ACTIVE)', 'lds', '%.1f'),
        ('  of which bank conflicts (SQ_LDS_BANK_CONFLICT)', 'conf', '%.1f'),
        ('SMEM / VMEM read / VMEM write instructions', None, None),
        ('SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES', 'wia', '%.3f'),
        ('SQ_WAIT_ANY / SQ_WAVE_CYCLES', 'wa', '%.3f'),
        ('SQ_WAIT_INST_LDS / SQ_WAVE_CYCLES', 'wil', '%.3f'),
        ('kernel time, ms (rocprofv3 --kernel-trace --stats, mean)', 'kt', '%.4f'),
        ('kernel time, ms (HIP events, unprofiled bench.py --full)', 'ev', '%.4f'),
        ('effective clock, GHz (GRBM_GUI_ACTIVE / 8 / kernel time)', 'clk', '%.2f'),
        ('bench value, 1e9 frames/s (this device; devices differ by +-5 %)', 'fps', '%.3f')]


def main():
    d, tag, what = sys.argv[1:4]
    c, v, b = read(d)
    cols = [(what, v)]
    if len(sys.argv) > 5:
        cols.insert(0, (sys.argv[5], read(sys.argv[4])[1]))
    out = ["Counters of %s on the bench workload (10 000 S-MFCC utterances, %d frames per launch)." % (v['kernel'], F),
           "rocprofv3 --pmc in separate passes (python3 bench.py --steps 3 --warmup 1 --no-cpu --no-extra), nothing traced beside them;",
           "kernel time from a rocprofv3 --kernel-trace --stats run of its own; same device, same run for all columns.", ""]
    for i, (w, _) in enumerate(cols):
        out.append("  column %d: %s" % (i + 1, w))
    out += ["", "Per frame:"]
    for name, key, fmt in ROWS:
        if key is None:
            out.append("  %-86s" % name + "".join("  %20s" % ("%.2f / %.2f / %.2f" % (x['smem'], x['vrd'], x['vwr'])) for _, x in cols))
        else:
            out.append("  %-86s" % name + "".join("  %20s" % (fmt % x[key]) for _, x in cols))
    out += ["", "Raw means per dispatch (last column's build):"] + ["  %-24s %.6g" % (k, c[k]) for k in sorted(c)]
    open('profiles/%s_pmc_summary.txt' % tag, 'w').write("\n".join(out) + "\n")
    shutil.copy(d + '/kernel_stats.csv', 'profiles/%s_bench_kernel_stats.csv' % tag)
    t = json.load(open('profiles/traffic.json'))
    t.update(kernel=v['kernel'], valu_instr_per_frame=round(v['valu'], 1), lds_cycles_per_frame=round(v['lds'], 1), hbm_bytes_per_frame=int(round(v['hbm'])),
             valu_issue_slots_per_frame=round(v['slots'], 1), clock_ghz=round(v['clk'], 2),
             source="profiles/%s_pmc_summary.txt, taken on %s (rocprofv3 --pmc, separate passes, bench.py --steps 3 --no-cpu --no-extra): "
                    "(2*FETCH_SIZE + WRITE_SIZE) KiB, SQ_INSTS_VALU, SQ_LDS_IDX_ACTIVE, GRBM_GUI_ACTIVE / 8 / kernel time, each / 9,009,528 frames; "
                    "valu_issue_slots_per_frame = %.1f - (%.1f - SQ_INSTS_VALU per frame): round 4's priced slots less the plain one-slot instructions "
                    "that have left phase 2 since (profiles/r04_frontend_cost_model.txt, tools/make_pmc_summary.py); counters are not collected "
                    "inside the timed run" % (tag, what, ANCHOR_SLOTS, ANCHOR_VALU))
    json.dump(t, open('profiles/traffic.json', 'w'), indent=1)
    print("\n".join(out[:len(cols) + 5 + len(ROWS) + 2]))


if __name__ == "__main__":
    main()
