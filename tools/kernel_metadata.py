"""Register and scratch metadata of the march / shade kernels in a built libovr_hip.so, read from its embedded code objects (no GPU): the table of
DESIGN.md section 12 and profiles/r09_clipping.md.

    python tools/kernel_metadata.py LIB                   one line per raymarch_kernel / shade_pool_kernel instantiation
    python tools/kernel_metadata.py LIB --against PARENT  every instantiation of PARENT must be in LIB with the same VGPRs, SGPRs, spilled scalars,
                                                          scratch and LDS (exit status 1 otherwise); the instantiations only LIB has are summarised
    --all                                                 every kernel of the library, not only the march / shade kernels; with --against the
                                                          kernels only PARENT has are listed by name (--removed N: exactly N of them are expected)

A template parameter appended behind the existing ones with the value `false` (how MAT, CLIP and ORTHO were added) renames every kernel: names are
compared with trailing `false` parameters removed - of the march and shade kernels, and of the projection, isosurface, schedule and shade-factor kernels,
which the orthographic camera gave such a parameter."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def read(lib, every=False):
    """mangled kernel name -> {field: value} for the march / shade kernels of lib, or for every kernel"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, capture_output=True, check=True)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=tmp, capture_output=True, text=True, check=True).stdout
            # one list item of amdhsa.kernels per kernel, its keys in alphabetical order: .group_segment_fixed_size stands BEFORE .name
            for item in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
                name, fields = None, {}
                for line in item.splitlines():
                    if not line.startswith("    ."):
                        line = "    " + line if line.startswith(".") else ""  # (the item's first key follows its dash)
                    line = line[4:]
                    if line.startswith(".name:"):
                        name = line.split(":", 1)[1].strip()
                    for k in FIELDS:
                        if line.startswith(k + ":"):
                            fields[k] = int(line.split(":")[1])
                if name:
                    out[name] = fields
    return {n: k for n, k in out.items() if every or "raymarch_kernel" in n or "shade_pool_kernel" in n}


def key(name):
    """the instantiation without trailing `false` template parameters"""
    m = re.match(r"(.*?(?:raymarch_kernel|shade_pool_kernel|project_kernel|isosurface_kernel|schedule_classify_kernel|shade_floats_kernel)I)((?:L[ib]\d+E)+)(E.*)", name)
    if not m:
        return name
    params = re.findall(r"L[ib]\d+E", m.group(2))
    while params and params[-1] == "Lb0E":
        params.pop()
    return m.group(1) + "".join(params) + m.group(3)


def params(name):
    m = re.match(r".*?(raymarch_kernel|shade_pool_kernel)I((?:L[ib]\d+E)+)E", name)
    return m.group(1), [int(x) for x in re.findall(r"L[ib](\d+)E", m.group(2))]


def rng(vals):
    vals = list(vals)
    return "-" if not vals else str(vals[0]) if min(vals) == max(vals) else f"{min(vals)}-{max(vals)}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--against")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--removed", type=int, default=0)
    a = ap.parse_args()
    mine = {key(n): k for n, k in read(a.lib, a.all).items()}
    # (the parser goes by the layout of llvm-readelf's output: a library that yields no kernel, or kernels without registers, was not understood)
    if not mine or any(".vgpr_count" not in k for k in mine.values()):
        raise SystemExit(f"{a.lib}: no kernel metadata understood ({len(mine)} names)")
    if not a.against:
        for n in sorted(mine):
            print(n, " ".join(f"{f[1:]}={mine[n].get(f, 0)}" for f in FIELDS))
        return 0
    parent = {key(n): k for n, k in read(a.against, a.all).items()}
    if not parent or any(".vgpr_count" not in k for k in parent.values()):
        raise SystemExit(f"{a.against}: no kernel metadata understood ({len(parent)} names)")
    removed = sorted(n for n in parent if n not in mine) if a.all else []
    changed = [n for n in parent if n not in removed and (n not in mine or mine[n] != parent[n])]
    new = sorted(set(mine) - set(parent))
    print(f"{len(parent)} instantiations in the parent, {len(parent) - len(changed) - len(removed)} with identical metadata here, {len(changed)} changed or missing")
    for n in changed:
        print("  CHANGED", n, parent[n], "->", mine.get(n))
    if a.all:
        print(f"{len(removed)} kernels of the parent are not here ({a.removed} expected)")
        for n in removed:
            print("  REMOVED", n)
    print(f"{len(new)} new instantiations; using scratch: {sum(1 for n in new if mine[n].get('.private_segment_fixed_size', 0) > 0)}")
    groups = {}
    for n in new:
        if "raymarch_kernel" not in n and "shade_pool_kernel" not in n:
            print("  NEW", n, mine[n])
            continue
        kern, p = params(n)
        p = p + [0] * (9 - len(p))
        g = (kern, p[1], "pooled" if kern == "raymarch_kernel" and p[3] else "", p[4] if kern == "raymarch_kernel" else p[3])
        groups.setdefault(g, []).append(mine[n])
    print("kernel | SHADE | | SKIP | n | VGPR | SGPR | spilled scalars | scratch")
    for g in sorted(groups):
        ks = groups[g]
        print(" | ".join([g[0], str(g[1]), g[2], str(g[3]), str(len(ks))] + [rng(k.get(f, 0) for k in ks) for f in (FIELDS[0], FIELDS[1], FIELDS[2], FIELDS[4])]))
    for n in new:
        if mine[n].get(".private_segment_fixed_size", 0) > 0:
            print("  SCRATCH", n, mine[n])
    return 1 if changed or len(removed) != a.removed or (a.all and new) else 0


if __name__ == "__main__":
    sys.exit(main())
