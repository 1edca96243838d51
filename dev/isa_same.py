"""Per-kernel comparison of two device assembly listings: python dev/isa_same.py PARENT.s NEW.s [--json OUT]

The listings come from build.py's flags plus `--cuda-device-only -S`, one per translation unit and side:

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fvisibility=hidden -Iinclude -Icuda.radixsort_amd/csrc \
          --cuda-device-only -S cuda.radixsort_amd/csrc/rsort_kernels.hip -o new/rsort_kernels.s

A kernel's text is its instructions and labels, from its label to its end label, with comments stripped and the
per-function numbers of local labels removed; the kernel descriptor (`.amdhsa_kernel` block) is not compared,
its figures come from the metadata and are shown for kernels that differ. One line per kernel: `same`, or
`differs` with VGPRs, SGPRs, scratch bytes, LDS bytes and instruction count of both sides (parent -> new).
Several pairs of listings: repeat the two arguments (P1.s N1.s P2.s N2.s ...). Exit status 1 if any differs.
"""
import json
import re
import subprocess
import sys


def kernels(path):
    """{symbol: (normalised text lines, meta dict)} of one listing."""
    text = open(path).read()
    meta = {}
    for blk in text.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
        meta[name] = {"vgpr": g("vgpr_count"), "sgpr": g("sgpr_count"), "scratch": g("private_segment_fixed_size"),
                      "lds": g("group_segment_fixed_size")}
    out = {}
    lines = text.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"(\w+):\s*; @\1\s*$", lines[i])
        if m is None or m.group(1) not in meta:
            i += 1
            continue
        name, body = m.group(1), []
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            s = lines[i].split(";")[0].rstrip()
            s = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", s)
            if s.strip() and not s.lstrip().startswith(".section"):
                body.append(s)
            i += 1
        meta[name]["insts"] = sum(1 for s in body if s[0] in " \t" and not s.lstrip().startswith("."))
        out[name] = (body, meta[name])
    return out


def main(argv):
    out_json = None
    if "--json" in argv:
        k = argv.index("--json")
        out_json = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    if len(argv) < 2 or len(argv) % 2:
        sys.exit(__doc__)
    rows, bad = [], 0
    for p, n in zip(argv[0::2], argv[1::2]):
        kp, kn = kernels(p), kernels(n)
        names = sorted(set(kp) | set(kn))
        dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        for name, d in zip(names, dem):
            if name not in kp or name not in kn:
                rows.append({"kernel": d, "result": "only in parent" if name in kp else "only in new"})
            elif kp[name][0] == kn[name][0]:
                rows.append({"kernel": d, "result": "same"})
            else:
                rows.append({"kernel": d, "result": "differs", "parent": kp[name][1], "new": kn[name][1]})
    for r in rows:
        if r["result"] == "differs":
            a, b = r["parent"], r["new"]
            print("differs  " + "  ".join(f"{k} {a[k]} -> {b[k]}" for k in ("vgpr", "sgpr", "scratch", "lds", "insts")) +
                  "  " + r["kernel"])
        else:
            print(f"{r['result']:8} {r['kernel']}")
        bad += r["result"] != "same"
    print(f"{len(rows)} kernels, {len(rows) - bad} same, {bad} not", file=sys.stderr)
    if out_json:
        json.dump({"kernels": len(rows), "same": len(rows) - bad, "not_same": [r for r in rows if r["result"] != "same"]},
                  open(out_json, "w"), indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
