#!/usr/bin/env python3
"""The program and the summary of tools/pmc_detector_lp.sh (how profiles/pmc_conv2d_lp.json is made).
  run [precision]   neck + head of the PointPillars configuration with `precision` (default fp16) four times on the seeded
                    468 x 468 canvas at B = 1: the program the counter passes run
  sum DIR OUT       the counters of every pass under DIR summed over the dispatches of each conv2d_lp_kernel instance -> OUT
                    (*_per_simd_cycle = counter / (1024 SIMDs x GRBM_GUI_ACTIVE / 8 XCDs))"""
import csv
import glob
import importlib
import json
import os
import re
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = (("SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAIT_INST_ANY", "SQ_WAIT_ANY"),
          ("SQ_INSTS_VALU", "SQ_INSTS_MFMA", "SQ_INSTS_LDS", "SQ_INSTS_SALU"),
          ("SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_ACTIVE_INST_LDS", "SQ_WAIT_INST_LDS"),
          ("SQ_VALU_MFMA_BUSY_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_VALU_MFMA_COEXEC_CYCLES", "GRBM_GUI_ACTIVE"))


def run(precision):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import rpn_ref as R
    rpn = importlib.import_module("3dal_pytorch_amd.rpn")
    neck, head = rpn.RPN(**R.NECK), rpn.CenterHead(**R.HEAD)
    neck.load_state_dict({k: torch.as_tensor(v) for k, v in R.neck_weights().items()}, strict=True)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in R.head_weights().items()}, strict=True)
    neck, head = neck.cuda().eval(), head.cuda().eval()
    neck.precision = head.precision = precision
    x = torch.from_numpy(R.canvas("bench1", (1, 64, 468, 468))).cuda()
    with torch.no_grad():
        for _ in range(4):
            head(neck(x))
    torch.cuda.synchronize()


def summarise(folder, out_path):
    out, disp = defaultdict(lambda: defaultdict(float)), defaultdict(set)
    for path in glob.glob(os.path.join(folder, "**", "*counter_collection.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                m = re.search(r"conv2d_lp_kernel<[^>]*>", row.get("Kernel_Name", ""))
                if not m:
                    continue
                for key in (m.group(0), "all conv2d_lp_kernel"):
                    out[key][row["Counter_Name"]] += float(row["Counter_Value"])
                disp[m.group(0)].add(row.get("Dispatch_Id"))
    res = {"_how": "bash tools/pmc_detector_lp.sh OUTDIR: one counter-only rocprofv3 --pmc pass per group of "
                   + " | ".join(" ".join(p) for p in PASSES) + " over `python3 tools/pmc_detector_lp.py run fp16` (MI355X)"}
    for k, v in out.items():
        r = dict(v)
        r["dispatches_per_pass"] = len(disp[k]) if k in disp else None
        if v.get("GRBM_GUI_ACTIVE"):
            cyc = v["GRBM_GUI_ACTIVE"] / 8
            for c in ("SQ_VALU_MFMA_BUSY_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS"):
                if c in v:
                    r[c + "_per_simd_cycle"] = v[c] / (1024 * cyc)
        if v.get("SQ_WAVE_CYCLES"):
            for c in ("SQ_WAIT_INST_ANY", "SQ_WAIT_ANY", "SQ_WAIT_INST_LDS", "SQ_BUSY_CYCLES"):
                if c in v:
                    r[c + "/SQ_WAVE_CYCLES"] = v[c] / v["SQ_WAVE_CYCLES"]
        if v.get("SQ_INSTS_MFMA"):
            r["LDS_per_MFMA"] = v.get("SQ_INSTS_LDS", 0) / v["SQ_INSTS_MFMA"]
            r["VALU_per_MFMA"] = (v.get("SQ_INSTS_VALU", 0) - v["SQ_INSTS_MFMA"]) / v["SQ_INSTS_MFMA"]
        res[k] = r
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    for k in sorted(res):
        if k != "_how":
            print(k, {a: round(b, 4) for a, b in res[k].items() if isinstance(b, float) and ("/" in a or "per" in a)})


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run(sys.argv[2] if len(sys.argv) > 2 else "fp16")
    elif len(sys.argv) == 4 and sys.argv[1] == "sum":
        summarise(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 2 and sys.argv[1] == "passes":
        print("\n".join(" ".join(p) for p in PASSES))
    else:
        sys.exit(__doc__)
