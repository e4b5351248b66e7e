#!/usr/bin/env python3
"""Are two device assembly files (hipcc --cuda-device-only -S) the same code, function by function?

    python profiles/isa_same.py parent.s candidate.s

A function is the text from its label up to its `.Lfunc_end`: the instructions and, for a kernel, the
`.amdhsa_kernel ... .end_amdhsa_kernel` descriptor.  Local labels carry the function's position in the file
(`.LBB12_3`, and `BB12_3` in the compiler's loop comments); the position is dropped, so functions that only moved compare equal.  Exit status 0: same set of
functions, every one identical.
"""
import re
import sys

BEGIN = re.compile(r"^([A-Za-z_$][\w$.]*):\s*; @")
END = re.compile(r"^\.Lfunc_end\d+:")
LOCAL = re.compile(r"\.L([A-Za-z_]+)\d+_(\d+)")
BLOCK_REF = re.compile(r"\bBB\d+_(\d+)")     # the same position in the compiler's comments ("in Loop: Header=BB12_3", "Child Loop BB12_7")


def functions(path):
    out, name, body = {}, None, []
    with open(path) as f:
        for line in f:
            if name is None:
                m = BEGIN.match(line)
                if m:
                    name, body = m.group(1), []
            elif END.match(line):
                out[name] = body
                name = None
            else:
                body.append(BLOCK_REF.sub(r"BB_\1", LOCAL.sub(r".L\1_\2", line.rstrip())))
    return out


def main(a_path, b_path):
    a, b = functions(a_path), functions(b_path)
    bad = sorted(set(a) ^ set(b))
    for n in bad:
        print("only in", a_path if n in a else b_path, ":", n)
    same = 0
    for n in sorted(set(a) & set(b)):
        if a[n] == b[n]:
            same += 1
            continue
        bad.append(n)
        first = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
        print(f"differs: {n}: {len(a[n])} -> {len(b[n])} lines, first difference at line {first} of the function")
    print(f"{same}/{len(set(a) | set(b))} functions identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
