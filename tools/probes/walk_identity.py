"""Are the rows of C2, C3 and C5 bit-identical between the in-tree library, the same library with the generic phase-2 walk forced
(CTU_PHASE2_GENERIC=1) and, when given, another build?   python tools/probes/walk_identity.py [other_lib.so]
300 / 300 / 60 S-MFCC utterances, device-resident runs, one child process per run."""
import os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
if len(sys.argv) > 1 and sys.argv[1] == "--child":
    import torch
    from ctucopy_amd import Engine, synth
    from tests.util import C2, C3, C5
    name, n, out = sys.argv[2], int(sys.argv[3]), sys.argv[4]
    eng = Engine({"C2": C2, "C3": C3, "C5": C5}[name])
    idx = list(range(n))
    plan = eng.plan(synth.lengths(synth.SET_SPEECH, idx))
    pcm = torch.from_numpy(np.asarray(synth.fill_arena(synth.SET_SPEECH, idx, plan.sample_off, plan.total_samples))).cuda()
    rows = eng.run_device(plan, pcm)
    torch.cuda.synchronize()
    np.save(out, rows.cpu().numpy())
else:
    other = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None
    ok = True
    for name, n in (("C2", 300), ("C3", 300), ("C5", 60)):
        runs = [("walk", {}), ("generic", {"CTU_PHASE2_GENERIC": "1"})] + ([("other", {"CTU_ENGINE_LIB": other})] if other else [])
        for tag, extra in runs:
            env = dict(os.environ)
            env.pop("CTU_PHASE2_GENERIC", None)
            env.update(extra)
            subprocess.run([sys.executable, __file__, "--child", name, str(n), "/tmp/walk_%s_%s.npy" % (name, tag)], check=True, env=env, timeout=300)
        a = np.load("/tmp/walk_%s_walk.npy" % name)
        for tag, _ in runs[1:]:
            b = np.load("/tmp/walk_%s_%s.npy" % (name, tag))
            same = a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
            ok &= same
            print(name, "rows", a.shape, "walk vs", tag, "bit-identical:", same, flush=True)
    sys.exit(0 if ok else 1)
