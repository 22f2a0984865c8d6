"""Records tests/golden/paircol_parent_rows.npz: the rows tests/test_frontend_paircol_gpu.py compares bit for bit.

Run on the GPU with an engine library built from the PARENT commit of the pair-column change, never with the code under test:

    git worktree add /tmp/parent <parent commit> && (cd /tmp/parent && tools/build_variant.sh parent)
    CTU_ENGINE_LIB=/tmp/parent/ctucopy_amd/_variants/lib_parent.so python tests/golden/make_paircol_parent_rows.py <parent commit> [out.npz]

The file holds this project's own outputs only: per configuration (C2, C3, C5) the rows of the short utterances of edge_utts() as
uint32 patterns, and a `how` entry that names the commit and the library they came from."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    lib = os.environ.get("CTU_ENGINE_LIB")
    assert lib and len(sys.argv) >= 2, __doc__
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "paircol_parent_rows.npz")
    from ctucopy_amd import Engine
    from tests.test_frontend_paircol_gpu import EDGE_CFG, EDGE_KERNEL, edge_utts
    z = {}
    for name, cfg in EDGE_CFG.items():
        eng = Engine(cfg)
        assert eng.kernel_name() == EDGE_KERNEL[name]
        for i, r in enumerate(eng.extract(edge_utts(name))):
            assert r.dtype == np.float32
            if not np.isfinite(r).all():  # recorded as they stand: bit patterns like any other
                print("%s utterance %d: %d nan, %d inf values" % (name, i, np.isnan(r).sum(), np.isinf(r).sum()))
            z["%s_%d" % (name, i)] = r.view(np.uint32).copy()
    z["how"] = np.array("rows of Engine(cfg).extract(edge_utts(name)) (tests/test_frontend_paircol_gpu.py) as uint32 patterns, written on an "
                        "MI355X by an engine library built with tools/build_variant.sh from the parent commit %s of the pair-column "
                        "change and loaded through CTU_ENGINE_LIB (%s)" % (commit, os.path.basename(lib)))
    np.savez_compressed(out, **z)
    print("wrote %s: %d arrays, %d bytes" % (out, len(z) - 1, os.path.getsize(out)))


if __name__ == "__main__":
    main()
