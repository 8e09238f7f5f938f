#!/usr/bin/env python3
"""Per-kernel resource and instruction counts of gfx950 assembly, two builds side by side.

    hipcc <the flags of videoyolo_amd/build.py> --cuda-device-only -S csrc/conv_split.hip -o new/conv_split.s
    (the same on a checkout of the commit to compare with, into parent/)
    python tools/asm_counts.py parent new conv_igemm conv_split conv_wino

One row per kernel symbol, every cell as `parent/new` (` *` where they differ): the registers, spills, scratch and LDS of
the kernel's metadata, and how many matrix, buffer, LDS-DMA, LDS and barrier instructions its text holds; then the count
of all instructions and whether the instruction text is the same.  Exit status 1 when a cell other than the last two
differs (profiles/conv_shared_parts.txt holds this tool's output).
"""
import re
import subprocess
import sys

META = [".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size"]
INSTR = ["v_mfma", "buffer_store", "buffer_load", "global_load_lds", "ds_read", "ds_write", "s_barrier"]


def kernels(path):
    text = open(path).read()
    out = {}
    # metadata: one YAML list entry per kernel
    for entry in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")])[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        out[name] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", entry).group(1)) for k in META}
    # text: from the symbol's label to its .Lfunc_end
    for name in out:
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M).group(0)
        lines = [l.strip() for l in body.splitlines()]
        for i in INSTR:
            out[name][i] = sum(1 for l in lines if l.startswith(i))
        out[name]["instructions"] = sum(1 for l in lines if re.match(r"(v|s|ds|buffer|global|flat|scratch)_", l))
        out[name]["text"] = "\n".join(l for l in lines if not l.startswith((";", ".")))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, r))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    parent, new, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    cols = META + INSTR + ["instructions"]
    differs = False
    for f in files:
        a, b = kernels("%s/%s.s" % (parent, f)), kernels("%s/%s.s" % (new, f))
        pretty = demangle(sorted(set(a) | set(b)))
        print("== %s.hip: %d kernels (parent) / %d (this change)" % (f, len(a), len(b)))
        same_text = 0
        for name in sorted(set(a) | set(b)):
            if name not in a or name not in b:
                print("%s: only in %s" % (pretty[name], "parent" if name in a else "this"))
                differs = True
                continue
            cells = []
            for c in cols:
                x, y = a[name][c], b[name][c]
                cells.append("%s %d/%d%s" % (c.lstrip("."), x, y, "" if x == y else " *"))
                differs |= x != y and c != "instructions"
            same = a[name]["text"] == b[name]["text"]
            same_text += same
            print("%s\n    %s | text %s" % (pretty[name], " | ".join(cells), "identical" if same else "differs"))
        print("-- %s.hip: instruction text identical for %d of %d kernels" % (f, same_text, len(b)))
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
