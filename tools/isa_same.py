#!/usr/bin/env python3
"""Is the device code of two builds the same, kernel by kernel?

    python tools/isa_same.py before/conv_l2-hip-amdgcn-amd-amdhsa-gfx950.s after/conv_l2-hip-amdgcn-amd-amdhsa-gfx950.s

Takes two device assembly files as `hipcc -save-temps` leaves them (build.py's flags) and compares, per function symbol, a
hash of its text from the label to the end-of-function marker: every instruction and the kernel descriptor block
(.amdhsa_kernel ... .end_amdhsa_kernel: registers, LDS, scratch).  Comments are dropped, and the function's running number
is taken out of local labels (.LBB<n>_<k>), so that a function added or removed elsewhere in the file flags nothing.
Prints one line per symbol that differs or exists on one side only, then the counts; exit status 1 unless all are identical.

A refactor that only moves device helpers between files should give "identical" for every kernel (docs/experiments.md,
"The limb format, once").  Check the tool on a build with one constant changed before believing a clean report.
"""
import hashlib
import re
import sys


def functions(path):
    """{symbol: sha256 of its normalised text}"""
    out, name, lines = {}, None, []
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].rstrip()  # the label line itself carries a trailing comment
        if name is None:
            m = re.match(r"^([A-Za-z_$][\w$.]*):$", line)
            if m and not line.startswith(".L"):
                name, lines = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:$", line):
            out[name] = hashlib.sha256("\n".join(lines).encode()).hexdigest()
            name = None
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.strip())
        if line:
            lines.append(line)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    same = 0
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            print(f"only in {sys.argv[2] if sym in b else sys.argv[1]}: {sym}")
        elif a[sym] != b[sym]:
            print(f"differs: {sym}")
        else:
            same += 1
    total = len(set(a) | set(b))
    print(f"{same} of {total} functions identical")
    return 0 if same == total and total > 0 else 1


if __name__ == "__main__":
    sys.exit(main())
