"""Record which form a table fill takes -- stb_default_variant, stb_fill_tuning's code, C, R and launches, and
stb_fill_takes_kind for kinds 1-3 -- for the shapes and settings of tests/test_fill_routes_host.py, as that test compares
them (test_the_reports_keep_the_recorded_routes).

  python tools/record_fill_routes.py --commit HASH [--out tests/golden/fill_routes.json]

Run it with the library built from the commit whose routes are to be kept (STB_LIB_PATH names another build), and name
that commit.  No GPU is needed: the reports launch nothing, and without a device the library counts 256 compute units.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_fill_routes_host as tfr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=tfr.GOLDEN)
    args = ap.parse_args()
    out = {"commit": args.commit, "columns": "default variant, form code, C, R, launches, takes kind 1, 2, 3",
           "routes": tfr.record()}
    with open(args.out, "w") as f:
        f.write("{\n \"commit\": %s,\n \"columns\": %s,\n \"routes\": {\n" % (json.dumps(out["commit"]), json.dumps(out["columns"])))
        f.write(",\n".join("  %s: {\n%s\n  }" % (json.dumps(n), ",\n".join("   %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rows.items()))
                           for n, rows in out["routes"].items()))
        f.write("\n }\n}\n")
    print("recorded %d settings x %d shapes of commit %s to %s" % (len(tfr.SETTINGS), len(tfr.SHAPES), args.commit, args.out))


if __name__ == "__main__":
    main()
