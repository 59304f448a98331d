#!/usr/bin/env python3
"""Write the fixture of a "bit-identical to the parent commit" test: SHA-256 of every tensor that the test module's cases produce, computed
with the library of the commit BEFORE a change that must not alter any bit (needs the GPU):

    tools/build_prev_lib.sh        # builds the last commit's sources beside the working tree's library
    E4S_LIB_PATH=$PWD/e4s_amd/libe4s_prev.so python tools/parent_digests.py tests/test_gpu_region_rows_bits.py [--out FILE]

The test module supplies everything -- GOLDEN (the fixture's path), GOLDEN_ENV (environment of its in-process cases), golden_cases()
({case id: arguments of run_case}), run_case, digests and, where it has cases that need a fresh process each, CHILD_MODES and
child_digests(mode) -- so the fixture and the test cannot drift apart (tests/test_gpu_wino1w_schedule.py,
tests/test_gpu_region_rows_bits.py).  With --check the digests of the loaded library are compared with the file instead of written."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("test_module", help="path of the test module, e.g. tests/test_gpu_wino1w_schedule.py")
    ap.add_argument("--out", help="default: the module's GOLDEN")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    name = os.path.splitext(os.path.basename(args.test_module))[0]
    spec = importlib.util.spec_from_file_location(name, os.path.abspath(args.test_module))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    os.environ.update(t.GOLDEN_ENV)
    from e4s_amd import lib
    doc = {"cases": {}}
    for cid, case_args in t.golden_cases().items():
        doc["cases"][cid] = t.digests(t.run_case(*case_args))
        print(cid, doc["cases"][cid], flush=True)
    if hasattr(t, "CHILD_MODES"):
        doc["children"] = {}
        for mode in t.CHILD_MODES:
            doc["children"][mode] = t.child_digests(mode)
            print("child", mode, doc["children"][mode], flush=True)
    out = args.out or t.GOLDEN
    if args.check:
        with open(out) as fh:
            want = json.load(fh)
        bad = [(sec, k) for sec in doc for k in doc[sec] if doc[sec][k] != want.get(sec, {}).get(k)]
        n = sum(len(doc[sec]) for sec in doc)
        print("library %s: %d of %d entries differ %s" % (os.path.basename(lib.LIB_PATH), len(bad), n, bad))
        return 1 if bad else 0
    doc["what"] = "SHA-256 of the output bytes of tests/%s.py's cases, from the library named below" % name
    doc["library"] = os.path.basename(lib.LIB_PATH)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
