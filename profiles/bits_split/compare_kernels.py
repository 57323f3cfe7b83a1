"""Kernel identity across a move between translation units: for every __global__ of the given units, the resource remarks and the
instruction sequence of two builds, matched by demangled name.

    hipcc <the flags of _build.py, without -shared> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage UNIT.hip -o DIR/UNIT.s 2> DIR/UNIT.remarks
    python compare_kernels.py BEFORE_DIR AFTER_DIR          # prints the table of RESULTS.md; exit status 1 if a kernel differs

Label numbers (.LBBf_n carries the function's index in its unit) and comments are stripped before the lines of a kernel - its
instructions and its kernel descriptor - are compared."""
import glob
import os
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def demangle(names):
    filt = os.environ.get("CXXFILT", "c++filt")
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def remarks(path):
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (.*) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = m.group(2)
    return res


def bodies(path, names):
    text = open(path).read()
    res = {}
    for n in names:
        m = re.search(r"^" + re.escape(n) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
        lines = [re.sub(r"\s+", " ", re.sub(r";.*", "", ln)).strip() for ln in m.group(1).split("\n")]
        res[n] = [re.sub(r"\.LBB\d+_", ".LBB_", ln) for ln in lines if ln]
    return res


def kernels(d):
    res = {}
    for rem in sorted(glob.glob(os.path.join(d, "*.remarks"))):
        r = remarks(rem)
        b = bodies(rem[:-len(".remarks")] + ".s", list(r))
        for mangled, plain in demangle(list(r)).items():
            assert plain not in res, plain
            res[plain] = (os.path.basename(rem)[:-len(".remarks")], r[mangled], b[mangled])
    return res


def main(before, after):
    a, b = kernels(before), kernels(after)
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    print("| kernel | unit before | unit after | lines | VGPRs | SGPRs | scratch | LDS | occupancy | resources | instructions |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    differs = 0
    for k in sorted(a, key=lambda k: (b[k][0], k)):
        (ua, ra, ia), (ub, rb, ib) = a[k], b[k]
        differs += ra != rb or ia != ib
        short = re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", k)
        print(f"| `{short}` | {ua} | {ub} | {len(ib)} | {rb['VGPRs']} | {rb['TotalSGPRs']} | {rb['ScratchSize [bytes/lane]']} | {rb['LDS Size [bytes/block]']} | "
              f"{rb['Occupancy [waves/SIMD]']} | {'identical' if ra == rb else 'DIFFERS'} | {'identical' if ia == ib else 'DIFFERS'} |")
    print(f"\n{len(a)} kernels, {differs} differ")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
