"""Record the output bits of the grouped and the tree base-weight step (stb_sample_hgroups, stb_sample_htree) on the cases
of tests/hh_oracle.py and tests/ht_oracle.py, as tests/test_gpu_hgroups.py and tests/test_gpu_htree.py compare them
(test_the_step_keeps_the_recorded_bits): hashes of the arrays, the concentrations' bit patterns, the totals.

  python tools/record_hstep_bits.py --commit HASH [--out tests/golden/hstep_bits.json] [--against FILE]

Run it with the library built from the commit whose bits are to be kept, and name that commit.  Counts are integers and a
row's normaliser is summed by one thread, so no bit depends on launch geometry or on the order of atomics: two runs give
the same file.  --against FILE compares with an earlier recording instead of trusting that, and fails on a difference.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hh_oracle as hho  # noqa: E402
import ht_oracle as hto  # noqa: E402
import test_gpu_hgroups as tgh  # noqa: E402
import test_gpu_htree as tgt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=tgh.BITS)
    ap.add_argument("--against", default=None)
    args = ap.parse_args()
    out = {"commit": args.commit, "hgroups": {}, "htree": {}}
    for name in hho.CASES:
        out["hgroups"][name] = tgh.bits_of(tgh.device_step(hho.case(name)))
    for name, flags in hto.STEPS:
        out["htree"]["%s/%d" % (name, flags)] = tgt.bits_of(tgt.device_step(hto.case(name, flags)))
    if args.against:
        with open(args.against) as f:
            old = json.load(f)
        diff = [(kind, k) for kind in ("hgroups", "htree") for k in out[kind] if out[kind][k] != old[kind].get(k)]
        print("differing cases:", diff)
        if diff:
            sys.exit(1)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("recorded %d grouped and %d tree steps of commit %s to %s" % (len(out["hgroups"]), len(out["htree"]), args.commit, args.out))


if __name__ == "__main__":
    main()
