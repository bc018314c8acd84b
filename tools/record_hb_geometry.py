"""Record the strip geometry of the halo-block fill and of the grid walk -- stb_fill_workspace_bytes, stb_fill_tuning's
code, C, R and launches, stb_grid_shape's status, C, G and K -- for the shapes, table counts and settings of
tests/test_hb_geometry_host.py, as that test compares them (test_the_reports_keep_the_recorded_geometry).

  python tools/record_hb_geometry.py --commit HASH [--out tests/golden/hb_geometry.json]

Run it with the library built from the commit whose geometry is to be kept (STB_LIB_PATH names another build), and name
that commit.  No GPU is needed: the reports launch nothing, and without a device the library counts 256 compute units.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_hb_geometry_host as thg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=thg.GOLDEN)
    args = ap.parse_args()
    columns = "workspace bytes, form code, C, R, launches, grid shape: status, C, G, K"
    geometry = thg.record()
    with open(args.out, "w") as f:
        f.write("{\n \"commit\": %s,\n \"columns\": %s,\n \"geometry\": {\n" % (json.dumps(args.commit), json.dumps(columns)))
        f.write(",\n".join("  %s: {\n%s\n  }" % (json.dumps(n), ",\n".join("   %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rows.items()))
                           for n, rows in geometry.items()))
        f.write("\n }\n}\n")
    print("recorded %d settings x %d shapes x %d table counts of commit %s to %s" %
          (len(thg.SETTINGS), len(thg.SHAPES), len(thg.TABLES), args.commit, args.out))


if __name__ == "__main__":
    main()
