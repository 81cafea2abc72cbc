#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of one kernel file, kernel by kernel (a refactor's proof
that the code did not move): the set of kernel symbols, per kernel the register counts, scratch,
spills, LDS, occupancy and the counts of MFMA / ds_read / LDS-DMA / s_barrier instructions, and
whether the instruction streams are identical.

  hipcc -std=c++17 -O3 --offload-arch=gfx950 --cuda-device-only -S -o old.s k_gemm.hip   (each tree)
  python tools/isa_compare.py old.s new.s [--json out.json]
Exit status 1 when the symbol sets differ."""
import json
import re
import sys

META = {"vgpr": r"; NumVgprs: (\d+)", "agpr": r"; NumAgprs: (\d+)", "scratch": r"; ScratchSize: (\d+)",
        "occupancy": r"; Occupancy: (\d+)", "lds": r"; LDSByteSize: (\d+)"}   # lds: static only (the GEMMs' is dynamic)
COUNTS = {"mfma": r"^v_mfma", "ds_read": r"^ds_read", "lds_dma": r"^global_load_lds", "s_barrier": r"^s_barrier"}


def kernels(path):
    text = open(path).read()
    out = {}
    # a kernel: from its label to the end of the metadata comment block after .Lfunc_end
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:\n", text, re.S | re.M):
        name, body, tail = m.group(1), m.group(2), text[m.end():m.end() + 4000]
        if ".amdhsa_kernel " + name not in text:
            continue
        ins = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") and not line.endswith(":"):
                continue
            ins.append(re.sub(r"\.L(BB|func_end|tmp)\d+_?", r".L\1_", line))   # labels carry the function's index
        k = {"ins": ins, "spills": len(re.findall(r"Folded Spill", body))}
        for key, pat in META.items():
            mm = re.search(pat, tail)
            k[key] = int(mm.group(1)) if mm else None
        for key, pat in COUNTS.items():
            k[key] = sum(1 for i in ins if re.match(pat, i))
        out[name] = k
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    report = {"symbols_equal": sorted(a) == sorted(b), "only_old": sorted(set(a) - set(b)),
              "only_new": sorted(set(b) - set(a)), "kernels": {}}
    keys = list(META) + ["spills"] + list(COUNTS)
    for name in sorted(set(a) & set(b)):
        ka, kb = a[name], b[name]
        same = ka["ins"] == kb["ins"]
        row = {"identical_stream": same, "instructions": [len(ka["ins"]), len(kb["ins"])]}
        for k in keys:
            row[k] = [ka[k], kb[k]]
        report["kernels"][name] = row
        moved = [f"{k} {ka[k]}->{kb[k]}" for k in keys if ka[k] != kb[k]]
        print(f"{'same' if same else 'DIFF'} {name} ins {len(ka['ins'])}->{len(kb['ins'])} vgpr {kb['vgpr']} agpr {kb['agpr']} "
              f"scratch {kb['scratch']} lds {kb['lds']} occ {kb['occupancy']} mfma {kb['mfma']} ds_read {kb['ds_read']} "
              f"dma {kb['lds_dma']} bar {kb['s_barrier']}" + (" | " + ", ".join(moved) if moved else ""))
    print(f"symbols equal: {report['symbols_equal']} ({len(a)} old, {len(b)} new); identical streams: "
          f"{sum(r['identical_stream'] for r in report['kernels'].values())} of {len(report['kernels'])}")
    if "--json" in sys.argv:
        json.dump(report, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
    return 0 if report["symbols_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
