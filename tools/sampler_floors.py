#!/usr/bin/env python
"""What float32 arithmetic costs the hierarchical sampler, case by case, without a device.

    python tools/sampler_floors.py --out profiles/sampler_floors_cpu.json

For every case of oracle/sampler_cases.py: F_z = max|z32 - z64| and F_cdf = max|cdf32 - cdf64| of oracle/sampler_ops.py's model in
float32 against float64, and how many entries are branch-sensitive at the class's tau (10 F_cdf tight, 3 F_cdf ill-conditioned).
tests/test_gpu_sampler.py recomputes the floors at run time; this record is what tests/test_sampler_model_cpu.py compares with.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import sampler_cases as sc      # noqa: E402
from oracle import sampler_ops as so        # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = {}
    for name in sc.upsample_case_names():
        case = sc.upsample_case(name)
        s64, s32 = so.stages_of(case, torch.float64), so.stages_of(case, torch.float32)
        F_z, F_cdf = so.floors(s64, s32)
        tau = (10.0 if case["cls"] == "tight" else 3.0) * F_cdf
        sens, _ = so.classify(s64, tau, case["exact_knots"])
        cases[name] = {"cls": case["cls"], "B": case["B"], "M": case["M"], "n_imp": case["n_imp"], "inv_s": case["inv_s"], "F_z": F_z,
                       "F_cdf": F_cdf, "tau": tau, "sensitive": int(sens.sum()), "entries": int(sens.numel())}
    doc = {"what": "float32 against float64 of oracle/sampler_ops.py on the cases of oracle/sampler_cases.py (CPU, torch %s)" % torch.__version__,
           "cases": cases}
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
