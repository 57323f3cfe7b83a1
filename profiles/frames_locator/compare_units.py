"""Kernel identity of this refactor: profiles/bits_split/compare_kernels.py with two changes.  Kernels are matched by unit and by
their demangled name up to the parameter list (components_kernel's second argument type was renamed, CompFrames -> FramesPlanes;
the three instance units define kernels of one name; a kernel's own mangled name in its lines reads <kernel>), and for a kernel that differs the line count and the resources of BOTH builds are printed.

    python compare_units.py BEFORE_DIR AFTER_DIR     # directories of UNIT.s / UNIT.remarks, made as compare_kernels.py says
"""
import glob
import importlib.util
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("compare_kernels", os.path.join(HERE, "..", "bits_split", "compare_kernels.py"))
ck = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ck)

COLS = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def by_name(d):
    """(unit, kernel name up to the parameter list) -> (unit, resources, lines)"""
    res = {}
    for rem in sorted(glob.glob(os.path.join(d, "*.remarks"))):
        unit = os.path.basename(rem)[:-len(".remarks")]
        r = ck.remarks(rem)
        body = ck.bodies(rem[:-len(".remarks")] + ".s", list(r))
        for mangled, plain in ck.demangle(list(r)).items():
            short = re.sub(r"^void |\(anonymous namespace\)::", "", plain)
            short = short[:short.index("(")] if "(" in short else short
            assert (unit, short) not in res, (unit, short)
            res[(unit, short)] = (unit, r[mangled], [ln.replace(mangled, "<kernel>") for ln in body[mangled]])
    return res


def main(before, after):
    a, b = by_name(before), by_name(after)
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    same_units, rows = {}, []
    for k in sorted(a):
        (ua, ra, ia), (ub, rb, ib) = a[k], b[k]
        same = ra == rb and ia == ib
        same_units.setdefault(ub, []).append(same)
        if not same:
            ndiff = sum(x != y for x, y in zip(ia, ib)) + abs(len(ia) - len(ib))
            rows.append(f"| `{k[1]}` | {ub} | {len(ia)} / {len(ib)} | " + " | ".join(f"{ra[c]} / {rb[c]}" for c in COLS) +
                        f" | {'identical' if ra == rb else 'DIFFER'} | {ndiff} |")
    print("| kernel | unit | lines | VGPRs | SGPRs | scratch | LDS | occupancy | resources | lines that differ in place |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows))
    print()
    for u, flags in sorted(same_units.items()):
        print(f"{u}: {len(flags)} kernels, {len(flags) - sum(flags)} differ")
    print(f"\n{len(a)} kernels, {len(rows)} differ (every value: before / after)")
    return 1 if rows else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
