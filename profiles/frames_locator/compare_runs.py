"""The speed rule of this refactor over the JSON documents of a feature's bench script, run parent, tree, parent, tree:

    python compare_runs.py DIR NAME [LINE_FILTER]     # reads DIR/NAME_parent_{1,2}.json and DIR/NAME_this_tree_{1,2}.json

A line (any dict with a ``median`` and a ``spread`` in the document, named by its path) passes when the tree's slower run is no slower
than the parent's slower run plus the margin; the margin is the largest spread the PARENT's own two runs show for that line, between
the runs or between the repetitions inside a run.  Prints the table of RESULTS.md (microseconds); exit status 1 if a line fails."""
import json
import sys


def lines(doc, path=()):
    if isinstance(doc, dict):
        if "median" in doc and "spread" in doc:
            yield ".".join(path), doc
            return
        for k, v in doc.items():
            yield from lines(v, path + (str(k),))


def main(d, name, only="", tree="this_tree"):
    runs = {who: [dict(lines(json.load(open(f"{d}/{name}_{who}_{i}.json")))) for i in (1, 2)] for who in ("parent", tree)}
    print(f"| line | parent 1 | parent 2 | {tree} 1 | {tree} 2 | margin | parent's slower + margin | {tree}'s slower | |")
    print("|---|---|---|---|---|---|---|---|---|")
    failed = 0
    for key in runs["parent"][0]:
        if only not in key:
            continue
        p1, p2 = (r[key] for r in runs["parent"])
        t1, t2 = (r[key] for r in runs[tree])
        margin = max(abs(p1["median"] - p2["median"]), p1["spread"], p2["spread"])
        bound, slower = max(p1["median"], p2["median"]) + margin, max(t1["median"], t2["median"])
        ok = slower <= bound
        failed += not ok
        short = key.replace("lines.", "").replace("shapes.", "").replace("lines_us.", "")
        print(f"| {short} | {p1['median']:.1f} ({p1['spread']:.1f}) | {p2['median']:.1f} ({p2['spread']:.1f}) | {t1['median']:.1f} ({t1['spread']:.1f}) | "
              f"{t2['median']:.1f} ({t2['spread']:.1f}) | {margin:.1f} | {bound:.1f} | {slower:.1f} | {'passes' if ok else 'SLOWER'} |")
    print(f"\n{failed} lines slower (median of a run, the spread of its repetitions in brackets)")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
