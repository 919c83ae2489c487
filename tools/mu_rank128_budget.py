#!/usr/bin/env python3
"""Register / scratch / LDS budget of the fused MU kernels of ranks 65 .. 128 (MT = 5 .. 8 rank tiles).

Reads the code-object metadata in the ISA that `make` keeps next to the objects (nn_fac_amd/csrc/build/k_mu3.s .. k_mu6.s: right
KL, right general beta, left KL, left general beta) and, for the dynamic LDS, asks the launchers' own arithmetic
(csrc/k_mu_plan.h through `tools/nnf_plan.cpp shm`, compiled on the fly with the host compiler).

    python tools/mu_rank128_budget.py          one line per instantiation, exit status 1 if one is over budget

Budget of gfx950: 512 unified VGPR + AGPR per lane at one 256-thread workgroup per CU, 160 KiB of LDS per workgroup, and no
private segment (a spill inside the chunk loop costs more than the whole MFMA work of a step).  Scalar registers that the
compiler parks in the lanes of a VGPR (`sgpr_spill_count`; the KL left kernel does it for a handful at its entry, where it
branches to one of its row-tile forms) touch no memory: they are printed, not counted against the budget.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nn_fac_amd", "csrc")
UNITS = {3: ("right", "KL"), 4: ("right", "GEN"), 5: ("left", "KL"), 6: ("left", "GEN")}
BM_OF = {"KL": 1, "GEN": 9}
MAX_REGS, MAX_LDS = 512, 160 * 1024

_NAME = re.compile(r"nnf_mu_(left|right)_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")


def expected():
    """(side, MT, REM, form, VEC) of every instantiation the dispatcher can select above rank 64."""
    full = [(side, mt, 0, form, vec) for side, form in UNITS.values() for mt in (5, 6, 7, 8) for vec in (0, 1)]
    return sorted(full + [("left", 6, 4, "KL", 1)])      # ranks 97 .. 100, KL, aligned X: four leftover ranks on the VALU pipe


def kernels_of(path):
    """{(side, MT, REM, form, VEC): metadata dict} of the fused kernels in one kept .s file."""
    text = open(path).read()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry)      # (the version list behind the kernels has entries without one)
        m = _NAME.search(name.group(1)) if name else None
        if not m:
            continue
        form = {v: k for k, v in BM_OF.items()}.get(int(m.group(4)))
        vals = {k: int(re.search(r"\.%s:\s+(\d+)" % k, entry).group(1))
                for k in ("agpr_count", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                          "group_segment_fixed_size")}
        out[(m.group(1), int(m.group(2)), int(m.group(3)), form, int(m.group(5)))] = vals
    return out


def launcher_lds():
    """{(MT, REM, form): bytes of dynamic LDS the launchers request} from csrc/k_mu_plan.h."""
    cxx = os.environ.get("CXX", "c++")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "nnf_plan")
        subprocess.run([cxx, "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tools", "nnf_plan.cpp"), "-o", exe], check=True)
        lines = subprocess.run([exe, "shm"], check=True, capture_output=True, text=True).stdout.split("\n")
    return {(int(a), int(b), c): int(d) for a, b, c, d in (l.split() for l in lines if l.strip())}


def table():
    """One row per expected instantiation: dict with side, mt, form, vec and the budget figures (None: not in the ISA)."""
    lds = launcher_lds()
    found = {}
    for part, (side, form) in UNITS.items():
        path = os.path.join(CSRC, "build", "k_mu%d.s" % part)
        if os.path.exists(path):
            found.update({k: v for k, v in kernels_of(path).items() if k[0] == side and k[3] == form})
    rows = []
    for side, mt, rem, form, vec in expected():
        k = found.get((side, mt, rem, form, vec))
        row = dict(side=side, mt=mt, rem=rem, form=form, vec=vec, found=k is not None)
        if k is not None:
            # (.vgpr_count is the lane's whole unified file on gfx90a and later: architectural VGPRs + AGPRs, the value of
            # .amdhsa_next_free_vgpr; .agpr_count is the accumulator share of it)
            row.update(regs=max(k["vgpr_count"], k["agpr_count"]), scratch=k["private_segment_fixed_size"],
                       spills=k["vgpr_spill_count"], sgpr_to_lane=k["sgpr_spill_count"],
                       lds=k["group_segment_fixed_size"] + lds[(mt, rem, form)])
            row["ok"] = (row["scratch"] == 0 and row["spills"] == 0 and row["regs"] <= MAX_REGS and row["lds"] <= MAX_LDS)
        rows.append(row)
    return rows


def main():
    bad = 0
    for row in table():
        if not row["found"]:
            print("%-5s mt=%d rem=%d %-3s vec=%d  MISSING" % (row["side"], row["mt"], row["rem"], row["form"], row["vec"]))
            bad += 1
            continue
        print("%-5s mt=%d rem=%d %-3s vec=%d  regs=%3d scratch=%d vgpr_spills=%d sgpr_to_lane=%d lds=%6d %s" % (
            row["side"], row["mt"], row["rem"], row["form"], row["vec"], row["regs"], row["scratch"], row["spills"], row["sgpr_to_lane"], row["lds"],
            "" if row["ok"] else "OVER BUDGET"))
        bad += 0 if row["ok"] else 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
