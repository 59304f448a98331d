#!/usr/bin/env python3
"""Did a source change alter the code of a kernel?  Static, no GPU needed.

    mkdir /tmp/old && git archive HEAD~ e4s_amd/csrc include | tar -x -C /tmp/old
    python tools/isa_compare.py /tmp/old/e4s_amd/csrc e4s_amd/csrc [conv_region.hip ...]

Compiles each .hip file of both trees (default: every file that both have and whose text, or the text of a header it can reach, differs)
to gfx950 assembly with the flags of e4s_amd/build.py, per-file flags included (tools/mfma_gap_report.py does the compiling and the
parsing), and prints per kernel whether the instruction text is identical.  Where it is not: the kernel's metadata side by side
(registers, spills, private segment, static LDS) and, for MFMA kernels, mfma_gap_report's summary of the main loop of both sides and
whether the per-gap instruction counts of the two loops are the same.  Exit status 1 if a kernel's metadata or main loop differs."""
import argparse
import contextlib
import io
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfma_gap_report as G  # noqa: E402


def bodies(text):
    """symbol -> the instruction text of each function (labels and directives included, comments and blank lines dropped)."""
    out = {}
    for m in re.finditer(r"^([A-Za-z_$][\w.$]*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines = [ln.split(";")[0].rstrip() for ln in m.group(2).splitlines()]
        out[m.group(1)] = "\n".join(ln for ln in lines if ln.strip())
    return out


def include_of(csrc):
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(csrc))), "include")
    return inc if os.path.isdir(inc) else None


def changed_files(old, new):
    """.hip files present in both trees; all of them if any header differs, else those whose own text differs."""
    read = lambda d, f: open(os.path.join(d, f), "rb").read() if os.path.isfile(os.path.join(d, f)) else None
    hips = sorted(f for f in os.listdir(new) if f.endswith(".hip") and os.path.isfile(os.path.join(old, f)))
    headers = {f for d in (old, new) for f in os.listdir(d) if f.endswith(".h")}
    if any(read(old, h) != read(new, h) for h in headers):
        return hips
    return [f for f in hips if read(old, f) != read(new, f)]


def compare(fname, old, new):
    """-> (report text, ok)"""
    buf = io.StringIO()
    texts = [G.compile_to_asm(os.path.join(d, fname), [], include_of(d))[1] for d in (old, new)]
    body, meta, loops = [bodies(t) for t in texts], [G.kernel_meta(t) for t in texts], [dict(G.kernels(t)) for t in texts]
    syms = sorted(set(meta[0]) | set(meta[1]) | set(body[0]) | set(body[1]))
    names = G.demangle(syms)
    same = [s for s in syms if body[0].get(s) is not None and body[0].get(s) == body[1].get(s) and meta[0].get(s) == meta[1].get(s)]
    ok = True
    print(f"# {fname}: {len(same)} of {len(syms)} functions identical (instruction text and metadata)", file=buf)
    for s in syms:
        if s in same:
            print(f"   identical   {names[s]}", file=buf)
            continue
        if s not in body[0] or s not in body[1]:
            print(f"   ONLY IN {'NEW' if s in body[1] else 'OLD'}   {names[s]}", file=buf)
            ok = False
            continue
        m0, m1 = meta[0].get(s, {}), meta[1].get(s, {})
        n0, n1 = body[0][s].count("\n") + 1, body[1][s].count("\n") + 1
        print(f"   DIFFERS     {names[s]}  ({n0} -> {n1} lines)", file=buf)
        for k in G.META_KEYS:
            flag = "" if m0.get(k) == m1.get(k) else "   <-- differs"
            ok &= not flag
            print(f"      {k:28s} {m0.get(k, '?'):>8} {m1.get(k, '?'):>8}{flag}", file=buf)
        if s in loops[0] and s in loops[1]:
            l0, l1 = G.main_loop(loops[0][s]), G.main_loop(loops[1][s])
            eq = l0[1:] == l1[1:]
            ok &= eq
            print(f"      main loop: blocks, branches, v_mfma and the per-gap VALU / LDS / global / scratch / wait / s_* counts "
                  f"{'identical' if eq else 'DIFFER'} ({l0[3]} v_mfma, {len(l0[4])} gaps)", file=buf)
            for side, txt, lp in (("old", texts[0], loops[0]), ("new", texts[1], loops[1])):
                with contextlib.redirect_stdout(buf):
                    print(f"      -- {side}")
                    G.report(s, names[s], lp[s], G.spill_meta(txt), False)
    return buf.getvalue(), ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_csrc")
    ap.add_argument("new_csrc")
    ap.add_argument("files", nargs="*", help=".hip file names (default: every file a change can have reached)")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    files = [os.path.basename(f) for f in args.files] or changed_files(args.old_csrc, args.new_csrc)
    with ThreadPoolExecutor(args.j) as ex:
        results = list(ex.map(lambda f: compare(f, args.old_csrc, args.new_csrc), files))
    for text, _ in results:
        sys.stdout.write(text)
    bad = [f for f, (_, ok) in zip(files, results) if not ok]
    print(f"# {len(files)} files compared; metadata or main loop differs in: {bad or 'none'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
