#!/usr/bin/env python3
"""What sits between consecutive MFMAs of a kernel's main loop (static; no GPU needed).

    python tools/mfma_gap_report.py e4s_amd/csrc/conv_wino1w.hip [--kernel SUBSTR] [--gaps] [-D...]

Compiles ONE .hip file to gfx950 assembly with the flags of e4s_amd/build.py (its per-file flags included) and, per kernel, takes the
innermost loop around the basic block with the most v_mfma (the unrolled K loop of the MFMA kernels here; more than one block or branch
in it means that something in the source compiled to control flow, which cuts the loop into several scheduling regions) and prints
  * per gap (the instructions between two consecutive v_mfma) the VALU / LDS / global / wait counts (--gaps: the whole list),
  * their histogram,
  * a modelled overrun: a kernel that runs ONE wave per SIMD has nothing else to cover a gap, and a gap lasts about
    max(32, sum of issue costs) cycles for v_mfma_f32_32x32x16_bf16.  overrun = sum over gaps of
    max(0, 8 [the MFMA] + 4 VALU (5 for v_cvt_pk*) + 2 ds_* + 4 global/buffer/flat + 1 s_* - 32), as a share of 32 cycles per gap.
    The ds_* and s_* weights are guesses, and the model knows nothing of waits that are not satisfied: it ranks schedules, the
    kernel trace measures them.  For kernels with two or more waves per SIMD the other wave covers a long gap; read their figure
    as "what one wave alone would lose".
  * scratch_ accesses between the kernel's first and last v_mfma, and the spill counts of its metadata.
It looks at v_*, ds_*, global_* / buffer_* / flat_*, scratch_*, s_waitcnt and other s_* only."""
import argparse
import collections
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_module():
    spec = importlib.util.spec_from_file_location("_e4s_build", os.path.join(ROOT, "e4s_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_to_asm(src, extra, include=None):
    """(flags, assembly text) of one .hip file; headers come from the file's own directory and from `include` (default: this tree's)."""
    b = _build_module()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.isfile(hipcc):
        hipcc = "hipcc"
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [hipcc, f"--offload-arch={b.ARCH}", "-O3", "-std=c++17", "-I" + (include or os.path.join(ROOT, "include")),
           "-I" + os.path.dirname(os.path.abspath(src))]
    cmd += b.PER_FILE_FLAGS.get(os.path.basename(src), []) + extra + ["--cuda-device-only", "-S", src, "-o", out]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if res.returncode != 0:
        sys.stderr.write(res.stdout.decode(errors="replace"))
        raise SystemExit("hipcc failed")
    text = open(out).read()
    os.unlink(out)
    return " ".join(cmd[1:-3]), text


def demangle(names):
    try:
        res = subprocess.run(["c++filt"] + names, stdout=subprocess.PIPE, check=True)
        return dict(zip(names, res.stdout.decode().splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kind(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_"):
        return "cvt" if op.startswith("v_cvt_pk") else "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "global"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return None


COST = {"valu": 4, "cvt": 5, "lds": 2, "global": 4, "scratch": 4, "wait": 1, "salu": 1}


def kernels(text):
    """(symbol, [blocks]); a block = (label, [opcodes]) in program order."""
    out = []
    cur, blocks, ops = None, None, None
    for line in text.splitlines():
        s = line.strip()
        if not s or s.startswith(";"):
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            lab = m.group(1)
            if lab.startswith(".L"):
                if cur is not None:
                    ops = []
                    blocks.append((lab, ops))
            elif not lab.startswith("."):
                cur, blocks, ops = lab, [], []
                blocks.append((lab, ops))
                out.append((cur, blocks))
            continue
        if s.startswith("."):
            if s.startswith(".end_amdhsa_kernel") or s.startswith(".section"):
                cur = None
            continue
        if cur is None:
            continue
        op = s.split()[0]
        if kind(op):
            ops.append(op + " " + s.split()[1] if op.startswith(("s_branch", "s_cbranch")) else op)
    return [(k, b) for k, b in out if any(kind(o) == "mfma" for _, bb in b for o in bb)]


META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size")


def kernel_meta(text):
    """symbol -> {key: value} for META_KEYS, from the amdhsa.kernels metadata."""
    res = {}
    for blk in re.split(r"\n\s+- (?=\.agpr_count:)", text)[1:]:
        g = lambda key: (re.search(r"\." + key + r":\s+(\S+)", blk) or [None, "?"])[1]
        res[g("name")] = {k: g(k) for k in META_KEYS}
    return res


def spill_meta(text):
    """symbol -> (sgpr spills, vgpr spills, private segment bytes)"""
    return {k: (m["sgpr_spill_count"], m["vgpr_spill_count"], m["private_segment_fixed_size"]) for k, m in kernel_meta(text).items()}


def main_loop(blocks):
    """(label, blocks, branches, v_mfma, [Counter of instruction kinds per gap]) of the kernel's main loop."""
    # the main loop: the innermost backward branch around the block with the most v_mfma
    nm = [sum(1 for o in b if kind(o) == "mfma") for _, b in blocks]
    main = nm.index(max(nm))
    labels = {lab: i for i, (lab, _) in enumerate(blocks)}
    lo, hi = main, main
    for j in range(main, len(blocks)):
        tgt = [labels[o.split()[1]] for o in blocks[j][1] if o.startswith(("s_branch", "s_cbranch")) and o.split()[1] in labels]
        back = [t for t in tgt if t <= main]
        if back:
            lo, hi = max(back), j
            break
    lab = blocks[lo][0] + (" .. " + blocks[hi][0] if hi > lo else "")
    ops = [o for _, b in blocks[lo:hi + 1] for o in b]
    nbr = sum(1 for o in ops if o.startswith(("s_branch", "s_cbranch")))
    pos = [i for i, o in enumerate(ops) if kind(o) == "mfma"]
    gaps = [collections.Counter(kind(o) for o in ops[a + 1:b]) for a, b in zip(pos, pos[1:])]
    return lab, hi - lo + 1, nbr, len(pos), gaps


def report(sym, pretty, blocks, spills, show_gaps):
    flat = [o for _, b in blocks for o in b]
    idx = [i for i, o in enumerate(flat) if kind(o) == "mfma"]
    scratch_between = sum(1 for o in flat[idx[0]:idx[-1]] if kind(o) == "scratch")
    lab, nblk, nbr, nmfma, gaps = main_loop(blocks)
    print(f"== {pretty}")
    sg, vg, priv = spills.get(sym, ("?", "?", "?"))
    print(f"   spills: {vg} VGPR + {sg} SGPR, private segment {priv} B; scratch_ accesses between the first and the last v_mfma: {scratch_between}")
    print(f"   main loop {lab}: {nblk} block(s), {nbr} branch(es), {nmfma} v_mfma, {len(gaps)} gaps")
    if not gaps:
        return
    nv = [g["valu"] + g["cvt"] for g in gaps]
    over = [max(0, 8 + sum(COST[k] * n for k, n in g.items()) - 32) for g in gaps]
    tot = {k: sum(g[k] for g in gaps) for k in ("valu", "cvt", "lds", "global", "scratch", "wait", "salu")}
    print(f"   in the gaps: VALU {tot['valu'] + tot['cvt']} (of them v_cvt_pk {tot['cvt']}), LDS {tot['lds']}, global {tot['global']}, "
          f"scratch {tot['scratch']}, s_waitcnt {tot['wait']}, other s_* {tot['salu']}")
    hist = collections.Counter(nv)
    print("   VALU per gap : gaps   " + "  ".join(f"{v}:{hist[v]}" for v in sorted(hist)))
    print(f"   gaps with 0 VALU {hist[0]}, with > 5 VALU {sum(1 for v in nv if v > 5)}, with > 7 VALU {sum(1 for v in nv if v > 7)}; "
          f"largest {sorted(nv, reverse=True)[:6]}")
    print(f"   modelled overrun {sum(over)} of {32 * len(gaps)} cycles = {100.0 * sum(over) / (32 * len(gaps)):.1f} %  "
          f"({sum(1 for o in over if o)} gaps over 32 cycles)")
    if show_gaps:
        print("   gap: VALU LDS global wait s_* | modelled cycles")
        for i, g in enumerate(gaps):
            cyc = 8 + sum(COST[k] * n for k, n in g.items())
            print(f"   {i:4d}: {g['valu'] + g['cvt']:3d} {g['lds']:3d} {g['global'] + g['scratch']:3d} {g['wait']:3d} {g['salu']:3d} | {cyc:3d}{' *' if cyc > 32 else ''}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source")
    ap.add_argument("--kernel", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--gaps", action="store_true", help="print every gap")
    ap.add_argument("--min-mfma", type=int, default=8, help="skip kernels whose main block has fewer MFMAs")
    args, extra = ap.parse_known_args()
    flags, text = compile_to_asm(os.path.abspath(args.source), extra)
    ks = kernels(text)
    names = demangle([k for k, _ in ks])
    spills = spill_meta(text)
    print(f"# {os.path.relpath(os.path.abspath(args.source), ROOT)}: hipcc {flags.replace(ROOT + os.sep, '')}")
    for sym, blocks in ks:
        if args.kernel not in names[sym]:
            continue
        if sum(1 for _, b in blocks for o in b if kind(o) == "mfma") < args.min_mfma:
            continue
        report(sym, names[sym], blocks, spills, args.gaps)


if __name__ == "__main__":
    main()
