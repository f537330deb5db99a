#!/usr/bin/env python3
"""The kernel resource table of scan_segments<MODE, KIND, SRC> (profiles/rNN/resource_usage.txt) from the compiler's own
remarks -- no GPU needed.  Make the remarks of this commit and of its parent with
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude --cuda-device-only \\
          -Rpass-analysis=kernel-resource-usage -c sjpeg_amd/csrc/scan_engine.hip -o /dev/null 2> remarks.txt
in each tree, then
    python tools/resource_table.py parent_remarks.txt remarks.txt > profiles/rNN/resource_usage.txt
Prints both tables in full, and for every instantiation of the parent whether it reports the same figures here."""
import re
import subprocess
import sys

KINDS = ["Encode", "Tap", "Histo", "Stats", "Error", "EncodeTrellis", "StatsTrellis", "EncodeReplay", "StatsCoef",
         "EncodeRagged", "HistoRagged", "StatsRagged", "ErrorRagged", "StatsTrellisRagged", "EncodeReplayRagged"]
SRCS = ["kSrcRgb24", "kSrcRgbx32", "kSrcPlanes", "kSrcRgbPlanar", "kSrcRgbPlanarF"]
MODES = {1: "420", 3: "444", 4: "400"}
FIELDS = [("VGPRs", r"\bVGPRs: (\d+)"), ("AGPRs", r"AGPRs: (\d+)"), ("SGPRs", r"TotalSGPRs: (\d+)"),
          ("scr", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
          ("sspill", r"SGPRs Spill: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")]


def parse(path):
    """{(kind, mode, src): figures} of the scan_segments instantiations in a remarks file"""
    text = open(path, errors="replace").read()
    names = sorted(set(re.findall(r"Function Name: (\S+)", text)))
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    demangled = dict(zip(names, plain))
    out = {}
    blocks = re.split(r"(?=Function Name: )", text)
    for b in blocks:
        m = re.match(r"Function Name: (\S+)", b)
        if not m:
            continue
        t = re.search(r"scan_segments<(\d+), (\d+), (\d+)>", demangled.get(m.group(1), ""))
        if not t:
            continue
        mode, kind, src = (int(x) for x in t.groups())
        fig = {}
        for key, pat in FIELDS:
            v = re.search(pat, b)
            fig[key] = int(v.group(1)) if v else -1
        out[(KINDS[kind], MODES.get(mode, str(mode)), SRCS[src])] = fig
    return out


def cell(f):
    if f is None:
        return "-"
    return (f"{f['VGPRs']:3d} VGPR {f['AGPRs']} AGPR {f['SGPRs']:3d} SGPR scr {f['scr']:4d} spill {f['sspill']}/{f['vspill']} "
            f"occ {f['occ']} LDS {f['lds']}")


def table(title, t):
    srcs = [s for s in SRCS if any(k[2] == s for k in t)]
    print(title)
    print(f"{'kind':<19s} mode | " + " | ".join(f"{s:<58s}" for s in srcs))
    for kind in sorted({k[0] for k in t}):
        for mode in ("400", "420", "444"):
            if not any(k[:2] == (kind, mode) for k in t):
                continue
            print(f"{kind:<19s} {mode:<4s} | " + " | ".join(f"{cell(t.get((kind, mode, s))):<58s}" for s in srcs))
    print()


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    parent, this = parse(sys.argv[1]), parse(sys.argv[2])
    same = [k for k in parent if this.get(k) == parent[k]]
    changed = [k for k in parent if k in this and this[k] != parent[k]]
    gone = [k for k in parent if k not in this]
    print("Kernel resource usage of scan_segments<MODE, KIND, SRC> for gfx950, from")
    print("  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude --cuda-device-only "
          "-Rpass-analysis=kernel-resource-usage -c sjpeg_amd/csrc/scan_engine.hip")
    print("on this commit and on its parent, both tables in full (tools/resource_table.py).  SGPR = TotalSGPRs, scr = scratch in")
    print("bytes per lane, spill = SGPRs spilled / VGPRs spilled, occ = waves per SIMD (= workgroups of 256 threads per CU), LDS")
    print('in bytes per workgroup.  "-": the dispatch does not instantiate that class for that kind.')
    print()
    print(f"instantiations: parent {len(parent)}, this commit {len(this)}; of the parent's, identical on this commit: "
          f"{len(same)}, changed: {len(changed)}, gone: {len(gone)}")
    for k in sorted(changed):
        print(f"  changed: {k[0]} {k[1]} {k[2]}: parent {cell(parent[k])}  ->  {cell(this[k])}")
    print()
    table("PARENT COMMIT", parent)
    table("THIS COMMIT", this)
    return 0


if __name__ == "__main__":
    sys.exit(main())
