"""Writes tests/golden/captions_<dims>_<case>.npz: the project's own oracle (oracle/ref_cpu.reward_forward) in fp32 and in
bf16 on the full prompts of the caption-scoring cases (tests/captions_util.py), every CustomOutput field per caption row.

    python tests/golden/make_golden_captions.py [tiny|2b] [one|multi]        (default: all four files)

The fp32 run at 2B dims takes minutes on a CPU, which is why the GPU tests read these files instead of running it;
tests/test_captions_host.py re-derives the tiny one-video file and compares bits.
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import captions_util as cu  # noqa: E402


def main(argv):
    dims_list = [a for a in argv if a in cu.DIMS] or list(cu.DIMS)
    cases = [a for a in argv if a in cu.CASES] or list(cu.CASES)
    for dims in dims_list:
        for case in cases:
            arrays = {}
            for name, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
                t0 = time.time()
                out = cu.oracle_outputs(dims, case, dtype)
                print(f"{dims} {case} {name}: {time.time() - t0:.0f} s, scores {np.round(out['score'], 4).tolist()}", flush=True)
                for k, v in out.items():
                    arrays[f"{name}_{k}"] = v
            np.savez(cu.golden_path(dims, case), **arrays)
            print("wrote", cu.golden_path(dims, case), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
