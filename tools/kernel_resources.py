"""Kernel resource table from hipcc's -Rpass-analysis=kernel-resource-usage remarks.

    hipcc ... -Rpass-analysis=kernel-resource-usage -o /dev/null x.hip 2> remarks.txt
    python tools/kernel_resources.py remarks.txt [other.txt]

One file: a markdown table (kernel, VGPRs, AGPRs, scratch bytes per lane, static LDS bytes, occupancy, VGPR and SGPR spills).  Two files: the kernels of
the first whose demangled name, with every `Geo<11>, ` template argument dropped, is also in the second, side by side — how a
build before and after a change that only added template parameters is compared; exit status 1 if any figure differs."""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("VGPRs Spill", "VGPR spills"), ("SGPRs Spill", "SGPR spills"))


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        for key, short in FIELDS:
            m = re.search(r"remark: .*\s" + re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name][short] = int(m.group(1))
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n") if names else []
    return {re.sub(r"^void ", "", d).replace("(TowerArgs)", "").replace("Geo<11>, ", "").replace("<Geo<11> >", "").replace("<Geo<11>>", ""): out[n] for n, d in zip(names, dem)}


def main():
    a = parse(sys.argv[1])
    cols = [s for _, s in FIELDS]
    if len(sys.argv) == 2:
        print("| kernel | " + " | ".join(cols) + " |\n|---|" + "---|" * len(cols))
        for k, v in a.items():
            print("| `%s` | " % k + " | ".join(str(v.get(c, "")) for c in cols) + " |")
        return 0
    b = parse(sys.argv[2])
    bad = 0
    print("| kernel | " + " | ".join(c + " before / after" for c in cols) + " |\n|---|" + "---|" * len(cols))
    for k, v in a.items():
        if k not in b:
            print("| `%s` | only in %s |" % (k, sys.argv[1]))
            bad = 1
            continue
        cells = []
        for c in cols:
            cells.append("%s / %s" % (v.get(c), b[k].get(c)))
            bad |= v.get(c) != b[k].get(c)
        print("| `%s` | " % k + " | ".join(cells) + " |")
    return int(bad)


if __name__ == "__main__":
    sys.exit(main())
