"""Hardware counters of the a_cost kernels (acost_kernel, acost_vjp_kernel) on the tools/acost_bench.py workload: one
`rocprofv3 --pmc` pass per counter group, each a child run of acost_bench.py (--child, one repetition), with no tracing
in the same run.  Per kernel: counters per launch, per wavefront, and the derived shares.

    python tools/acost_pmc.py --variant 0 --out profiles/acost_pmc.json
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = [
    "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR",
    "SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT",
    "FETCH_SIZE", "WRITE_SIZE", "GRBM_GUI_ACTIVE",
]


def run_group(exe, group, variant, out):
    cmd = [exe, "--pmc", *group.split(), "--output-format", "csv", "-d", out, "--", sys.executable,
           os.path.join(HERE, "acost_bench.py"), "--child", "--reps", "1", "--warmup", "0", "--variant", str(variant)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    return r.returncode, r.stderr[-1500:]


def summarize(root):
    acc = {}
    for path in glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(path, newline="")):
            name = row["Kernel_Name"].split("(")[0].split("::")[-1]
            if "acost" not in name:
                continue
            d = acc.setdefault(name, {}).setdefault(row["Counter_Name"], {})
            d[row["Dispatch_Id"]] = d.get(row["Dispatch_Id"], 0.0) + float(row["Counter_Value"])
            acc[name].setdefault("_res", dict(lds=row.get("LDS_Block_Size"), scratch=row.get("Scratch_Size"),
                                              grid=row.get("Grid_Size"), vgpr=row.get("VGPR_Count")))
    out = {}
    for name, counters in acc.items():
        rec = {"resources": counters.pop("_res")}
        mean = {c: sum(v.values()) / len(v) for c, v in counters.items()}
        rec["per_launch"] = mean
        w = mean.get("SQ_WAVES")
        if w:
            pw = {c: v / w for c, v in mean.items() if c.startswith("SQ_") and c != "SQ_WAVES"}
            rec["per_wave"] = pw
            d = {}
            if "SQ_WAVE_CYCLES" in pw:
                # SQ_WAVE_CYCLES / SQ_ACTIVE_* / SQ_WAIT_* count in the same units per wave: their ratios are what matter
                for k in ("SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_ACTIVE_INST_ANY", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY",
                          "SQ_WAIT_INST_LDS"):
                    if k in pw:
                        d[k.lower().replace("sq_", "") + "_share_of_wave_cycles"] = pw[k] / pw["SQ_WAVE_CYCLES"]
            if "SQ_LDS_BANK_CONFLICT" in pw and "SQ_ACTIVE_INST_LDS" in pw and pw["SQ_ACTIVE_INST_LDS"] > 0:
                d["lds_bank_conflict_cycles_per_lds_active_cycle"] = pw["SQ_LDS_BANK_CONFLICT"] / pw["SQ_ACTIVE_INST_LDS"]
            if "SQ_WAVE_CYCLES" in mean and "GRBM_GUI_ACTIVE" in mean and mean["GRBM_GUI_ACTIVE"] > 0:
                # wave-cycles summed over the device per GPU-busy cycle: the mean number of resident wavefronts (in the
                # counters' units; compare kernels with each other, not with a hardware maximum)
                d["resident_waves_indicator"] = mean["SQ_WAVE_CYCLES"] / mean["GRBM_GUI_ACTIVE"]
            rec["derived"] = d
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", type=int, choices=(0, 1), default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    exe = shutil.which("rocprofv3")
    if not exe:
        sys.exit("rocprofv3 not found")
    tmp = tempfile.mkdtemp(prefix="acost_pmc_")
    failed = {}
    for i, g in enumerate(GROUPS):
        rc, err = run_group(exe, g, a.variant, os.path.join(tmp, "pmc%d" % i))
        if rc != 0:
            failed[g] = {"rc": rc, "stderr": err}
    res = {"workload": "tools/acost_bench.py --variant %d (65 536 knot-level scenario_1 candidates, per-candidate and shared "
                       "reference lines), one repetition per pass" % a.variant, "groups": GROUPS, "failed": failed,
           "kernels": summarize(tmp)}
    shutil.rmtree(tmp, ignore_errors=True)
    txt = json.dumps(res, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
