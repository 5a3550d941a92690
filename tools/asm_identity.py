"""Instruction identity of two builds of one translation unit, from the device assembly that `hipcc -save-temps=obj` leaves next to the object
(<unit>-hip-amdgcn-amd-amdhsa-gfx950.s); no GPU.

    python tools/asm_identity.py PARENT.s MINE.s [--removed N]

Every function (kernel or not) is compared by its symbol: the sequence of its instructions and directives with comments dropped and the basic-block
labels (.LBB<function>_<block>) renumbered relative to the function, since a function's number shifts when others leave the unit.  The __hip_cuid_<hash>
symbol - a hash over the source file's path - is ignored.  Exit status 1 if a function both builds have differs, if MINE has a function PARENT has
not, or if the number of PARENT's functions missing from MINE is not N (default 0); the missing ones are listed.  What stands outside the functions -
the kernel descriptors (registers, scratch, LDS) among it - is not compared here: tools/kernel_metadata.py --all compares those."""
import argparse
import re
import sys


def functions(path):
    """symbol -> normalised lines of its body"""
    funcs, name, body = {}, None, None
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].rstrip()
            if not line.strip() or "__hip_cuid_" in line:
                continue
            m = re.match(r"\s*\.type\s+(\S+),@function", line)
            if m:
                name, body = m.group(1), []
                continue
            if name is not None:
                if re.match(r"\s*\.size\s+" + re.escape(name) + ",", line):
                    funcs[name] = body
                    name = body = None
                    continue
                if re.match(r"\.Lfunc_(begin|end)\d+:", line):
                    continue
                body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line.strip()))
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("mine")
    ap.add_argument("--removed", type=int, default=0)
    a = ap.parse_args()
    parent = functions(a.parent)
    mine = functions(a.mine)
    missing = sorted(set(parent) - set(mine))
    new = sorted(set(mine) - set(parent))
    differ = sorted(n for n in parent if n in mine and parent[n] != mine[n])
    n_ins = sum(len(parent[n]) for n in parent if n in mine)
    print(f"{len(parent)} functions in the parent, {len(mine)} here; {len(parent) - len(missing) - len(differ)} identical ({n_ins} lines compared), "
          f"{len(differ)} differ, {len(missing)} missing, {len(new)} new")
    for n in differ:
        k = next((i for i, (x, y) in enumerate(zip(parent[n], mine[n])) if x != y), min(len(parent[n]), len(mine[n])))
        print(f"  DIFFERS {n}: {len(parent[n])} -> {len(mine[n])} lines, first at {k}")
    for n in missing:
        print("  MISSING", n)
    for n in new:
        print("  NEW", n)
    return 1 if differ or new or len(missing) != a.removed else 0


if __name__ == "__main__":
    sys.exit(main())
