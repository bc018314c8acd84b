"""Record the bytes of the table fills and the doubles of the fused evaluations of tests/test_gpu_fill_bits.py, as that
test compares them: a SHA-256 of each slab's stored cells (and of S1), the evaluations' results in hex.

  python tools/record_fill_bits.py --commit HASH [--out tests/golden/fill_bits.json] [--against FILE]

Run it on a GPU with the library built from the commit whose bits are to be kept (STB_LIB_PATH names another build), and
name that commit.  Run it twice, the second time with --against the first recording: a fill is deterministic by
construction, so a fill case that differs between the two runs is an error and nothing is written; a fused evaluation
that differs (its partial sums may come in another order) is recorded with "exact": false, and the test then compares it
at 1e-10.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_fill_bits as tfb  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=tfb.GOLDEN)
    ap.add_argument("--against", default=None)
    args = ap.parse_args()
    out = {"commit": args.commit, "fill": {}, "fused": {}}
    for name in tfb.FILLS:
        out["fill"][name] = tfb.fill_bits(name)
    for name in tfb.FUSED:
        values, form = tfb.fused_values(name)
        out["fused"][name] = {"exact": True, "form": form, "hex": tfb.hexes(values)}
    if args.against:
        with open(args.against) as f:
            old = json.load(f)
        diff = [k for k in out["fill"] if out["fill"][k] != old["fill"].get(k)]
        print("fill cases that differ between the two recordings:", diff)
        if diff:
            sys.exit(1)
        for k, v in out["fused"].items():
            if v["hex"] != old["fused"][k]["hex"] or not old["fused"][k]["exact"]:
                print("fused case %r differs between the two recordings: to be compared at 1e-10" % k)
                v["exact"] = False
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("recorded %d fills and %d fused evaluations of commit %s to %s" % (len(out["fill"]), len(out["fused"]), args.commit, args.out))


if __name__ == "__main__":
    main()
