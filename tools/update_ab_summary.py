"""Counter breakdown of the Schur update kernel's forms: turns the rocprofv3 --pmc csv directories of
`tools/micro/update_ab M K <form>` (one directory per form, one sub-directory per counter pass) into one JSON file.

    python tools/update_ab_summary.py out.json FORM=DIR [FORM=DIR ...] [--kernel gemm_nt_update_fast]

Per form and per launch: every counter's mean, the launch time under each pass, the wait / issue-stall / active shares
of the wave cycles, the LDS bank-conflict share of the LDS-active cycles, HBM traffic (FETCH_SIZE doubled, the gfx950
correction tools/pmc_summary.py applies), and the MFMA-busy fraction and effective clock computed as
tools/pmc_c4_post.py computes them."""
import csv
import glob
import json
import os
import sys
from collections import defaultdict


def one_form(d, kernel):
    acc, dur, cnt = defaultdict(float), defaultdict(float), defaultdict(int)
    names = set()
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if kernel not in r.get("Kernel_Name", ""):
                continue
            names.add(r["Kernel_Name"][:120])
            c = r.get("Counter_Name")
            acc[c] += float(r.get("Counter_Value", 0.0))
            dur[c] += (float(r.get("End_Timestamp", 0)) - float(r.get("Start_Timestamp", 0))) * 1e-6
            cnt[c] += 1
    row = {"kernel": sorted(names), "launches": {c: cnt[c] for c in sorted(cnt)}}
    per = {c: acc[c] / cnt[c] for c in acc}
    ms = {c: dur[c] / cnt[c] for c in acc}
    row["per_launch"] = {c: per[c] for c in sorted(per)}
    row["ms_under"] = {c: ms[c] for c in sorted(ms)}
    wc = per.get("SQ_WAVE_CYCLES")
    if wc:
        for c in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_WAIT_INST_LDS"):
            if c in per:
                row[c + "_share_of_wave_cycles"] = per[c] / wc
    if per.get("SQ_LDS_IDX_ACTIVE") and "SQ_LDS_BANK_CONFLICT" in per:
        row["lds_bank_conflict_share_of_lds_active"] = per["SQ_LDS_BANK_CONFLICT"] / per["SQ_LDS_IDX_ACTIVE"]
    if "FETCH_SIZE" in per:
        row["fetch_bytes_x2_corrected_per_launch"] = per["FETCH_SIZE"] * 1024.0 * 2.0
    if "WRITE_SIZE" in per:
        row["write_bytes_per_launch"] = per["WRITE_SIZE"] * 1024.0
    busy, active = per.get("SQ_VALU_MFMA_BUSY_CYCLES"), per.get("GRBM_GUI_ACTIVE")
    if busy and active:
        # SQ_VALU_MFMA_BUSY_CYCLES: summed over the chip's SIMD quads in units of 4 cycles; GRBM_GUI_ACTIVE: over 8 XCDs
        row["mfma_pipe_busy_fraction"] = busy / (active * 128.0)
        row["effective_clock_ghz"] = active / 8.0 / (ms["GRBM_GUI_ACTIVE"] * 1e-3) / 1e9
    return row


def main():
    args = sys.argv[1:]
    kernel = "gemm_nt_update_fast"
    if "--kernel" in args:
        i = args.index("--kernel")
        kernel = args[i + 1]
        del args[i:i + 2]
    out = args.pop(0)
    res = {"command": "rocprofv3 --pmc <one pass> --kernel-trace --output-format csv -d DIR/pN -- update_ab M K FORM",
           "forms": {}}
    for a in args:
        form, d = a.split("=", 1)
        res["forms"][form] = one_form(d, kernel)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
