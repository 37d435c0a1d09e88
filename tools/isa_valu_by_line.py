"""Static VALU count of one kernel by source line, from an assembly dump with
line tables (diagnostics, no GPU needed):

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -gline-tables-only -S \
        entropy_coders_amd/csrc/fse_decode_seg.hip -o dec.s
    python tools/isa_valu_by_line.py dec.s decode_pre_kernelILi11ELj45056ELi2ELi1ELj512 [SOURCE_DIR]

Every `v_*` instruction between the kernel's label and its end is charged to
the innermost `.loc` in force (an inlined callee's own line); with SOURCE_DIR
the line's text is printed beside its count.  The counts are static: a line
inside a loop counts once per copy the compiler made, not once per trip.
DESIGN.md section 5 (decode set-up table) weighs them by the flagship shape."""
import os
import re
import sys
from collections import Counter


def main():
    path, kernel = sys.argv[1], sys.argv[2]
    srcdir = sys.argv[3] if len(sys.argv) > 3 else None
    files, counts, inside, loc = {}, Counter(), False, None
    total = 0
    for ln in open(path, errors="replace"):
        s = ln.strip()
        m = re.match(r'\.file\s+(\d+)\s+(?:"([^"]*)"\s+)?"([^"]*)"', s)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3))
            continue
        if not inside:
            inside = s.startswith("_Z") and ":" in s and kernel in s.split(":")[0]  # the label, before its comment
            continue
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            loc = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
        elif s.startswith("v_"):
            counts[loc] += 1
            total += 1
    text = {}
    if srcdir:
        for name in {f for f, _ in counts if f}:
            p = os.path.join(srcdir, name)
            if os.path.exists(p):
                text[name] = open(p, errors="replace").read().splitlines()
    for (name, line), c in sorted(counts.items()):
        src = text.get(name, [])
        print(f"{c:5d}  {name}:{line}  {src[line - 1].strip()[:90] if 0 < line <= len(src) else ''}")
    print(f"{total:5d}  total VALU (static)")


if __name__ == "__main__":
    main()
