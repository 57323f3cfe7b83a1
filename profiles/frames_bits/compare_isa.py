"""Compare the kernels of two `hipcc -S --cuda-device-only` outputs of one translation unit, kernel by kernel.

    python profiles/frames_bits/compare_isa.py PARENT.s NEW.s [REMARKS]

Per kernel symbol: `same` when the instruction stream (every line between the symbol's label and its .Lfunc_end, comments and
local-label numbering aside) is identical in both files, `differs` with the number of differing lines otherwise, `new` / `gone` for
symbols only one file has.  REMARKS: the stderr of a compile with -Rpass-analysis=kernel-resource-usage - the VGPRs, scratch and
occupancy of the `new` kernels are then printed next to them."""
import re
import sys


def norm(t):
    """local labels carry a per-file function number (.LBB<n>_) and a per-file counter (.Lpost_getpc<n>): drop both"""
    return re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", t))


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            t = line.split(";")[0].strip()
            if t and not t.startswith("."):
                body.append(norm(t))
            elif t.startswith(".LBB"):
                body.append(norm(t))
    return out


def resources(path):
    res, name = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill): (\d+)", line)
        if m and name:
            res[name][m.group(1).split(" [")[0].replace(" ", "")] = int(m.group(2))
    return res


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    res = resources(sys.argv[3]) if len(sys.argv) > 3 else {}
    same = differs = 0
    for k in sorted(set(a) | set(b)):
        if k not in b:
            print(f"gone     {k}")
        elif k not in a:
            r = res.get(k, {})
            print(f"new      {k}  {len(b[k])} instructions  " + " ".join(f"{n}={v}" for n, v in r.items()))
        elif a[k] == b[k]:
            same += 1
        else:
            differs += 1
            import difflib
            d = [l for l in difflib.unified_diff(a[k], b[k], lineterm="", n=0) if l[0] in "+-" and not l.startswith(("+++", "---"))]
            print(f"differs  {k}  {len(d)} lines")
            for l in d[:12]:
                print("           " + l)
    print(f"{same} kernels same, {differs} differ")


if __name__ == "__main__":
    main()
