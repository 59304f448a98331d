#!/usr/bin/env python3
"""Write tests/golden/wino1w_parent_digests.json: SHA-256 of every tensor that the cases of tests/test_gpu_wino1w_schedule.py produce, computed
with the library of the commit BEFORE a scheduling change to csrc/conv_wino1w.hip (needs the GPU):

    git stash                      # or check the parent commit out: build_prev_lib.sh builds HEAD
    tools/build_prev_lib.sh && git stash pop
    E4S_LIB_PATH=$PWD/e4s_amd/libe4s_prev.so python tools/wino1w_parent_digests.py [--out FILE]

The cases, seeds and the launch are the test's own (imported from it), so the fixture and the test cannot drift apart.  With --check the
digests of the loaded library are compared with the file instead of written."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wino1w_parent_digests.json"))
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    os.environ["E4S_WINO_1W"] = "1"
    spec = importlib.util.spec_from_file_location("_wino1w_cases", os.path.join(ROOT, "tests", "test_gpu_wino1w_schedule.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    from e4s_amd import lib
    cases = {}
    for shape in t.SHAPES:
        for mode in t.MODES:
            cases[t.case_id(shape, mode)] = t.digests(t.run_case(shape, mode))
            print(t.case_id(shape, mode), cases[t.case_id(shape, mode)], flush=True)
    if args.check:
        with open(args.out) as fh:
            want = json.load(fh)["cases"]
        bad = [k for k in cases if cases[k] != want.get(k)]
        print("library %s: %d of %d cases differ %s" % (os.path.basename(lib.LIB_PATH), len(bad), len(cases), bad))
        return 1 if bad else 0
    doc = {"what": "SHA-256 of the output bytes of tests/test_gpu_wino1w_schedule.py's cases, from the library named below",
           "library": os.path.basename(lib.LIB_PATH), "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
