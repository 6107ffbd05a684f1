"""Writes tests/golden/chain_reads_first_off.npz, the vectors tests/test_gpu_chain_reads_first.py compares against: the outputs
of the library built WITHOUT the reads-first panel chain.
  MMX_BUILD_VARIANT=chainoff python -m momentum_amd.build
  MMX_LIB=$PWD/momentum_amd/libmmx_hip_chainoff.so python scripts/gen_chain_golden.py [out.npz]
(needs a GPU; MMX_LIB must name that library -- the script refuses the default one)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import test_gpu_chain_reads_first as t  # noqa: E402

if __name__ == "__main__":
    if "chainoff" not in os.environ.get("MMX_LIB", ""):
        sys.exit("MMX_LIB must name the chainoff library")
    out = {}
    for name in t.CASES:
        got = t.compute(torch, name)
        print(name, "n", int(got["n"]), "status", got["status"].tolist(), "smallest pivot ratio", got["diag"][:, 1].tolist())
        for key, val in got.items():
            out[f"{name}/{key}"] = np.asarray(val)
    path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    np.savez(path, **out)
    print("wrote", path)
