"""Child process of tests/test_nj_bootstrap_gpu.py::test_results_do_not_depend_on_the_batch: started with LDW_NJ_BATCH=4, it runs the same bootstrap at
that batch size, at LDW_NJ_BATCH=1 and without the variable (the library reads it at every call) and saves the three sets of outputs.

    python nj_boot_worker.py IN.npz OUT.npz        IN: states uint8 [L, N], mult int32 [B, L]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldweaver_amd.engine import Engine                     # noqa: E402


def main(src, dst):
    assert os.environ.get("LDW_NJ_BATCH") == "4"
    inp = np.load(src)
    out = {}
    with Engine(0) as eng:
        eng.set_alignment(inp["states"])
        for tag, value in (("b4", "4"), ("b1", "1"), ("default", None)):
            if value is None:
                del os.environ["LDW_NJ_BATCH"]
            else:
                os.environ["LDW_NJ_BATCH"] = value
            for name, a in zip(("parent", "length", "support", "rep_parent", "rep_length"), eng.nj_bootstrap(inp["mult"], want_trees=True)):
                out[f"{tag}_{name}"] = a
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
