#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device assemblies of csrc/emd.hip (runs without a GPU).

    hipcc <FLAGS of build.py without -fPIC> --cuda-device-only -S -o before.s csrc/emd.hip      (on the parent commit)
    hipcc <the same>                                            -o after.s  csrc/emd.hip
    python tools/emd_isa_compare.py before.s after.s > profiles/<name>.md

For a change that is meant to leave the device code alone.  Kernels are paired by base name and template arguments; a kernel whose
template argument list got shorter is paired with the parent instance whose leading arguments agree.  Each pair is classified:

  A  identical instruction text (comments, directives and label numbering aside).
  B  same work, other bookkeeping.  The kernel is reduced to the mnemonics, in program order, of its vector, LDS, global-memory,
     scratch and barrier instructions (v_* except v_mov*, ds_*, global_*, scratch_*, s_barrier) and of the record loads
     (s_load_dwordx8 / x16).  Then (i) between the first and the last s_load_dwordx16 — the sweep loop with its preload — that
     sequence is identical; (ii) over the whole kernel every such mnemonic occurs equally often, except that v_writelane_b32 /
     v_readlane_b32 may be fewer; (iii) the VGPR / SGPR / LDS / scratch / accum-offset lines of the kernel descriptor are identical.
     A kernel without s_load_dwordx16 has no (i).
  C  anything else; the failing conditions and the loop's mnemonic diff are printed.

Exit status 1 if any kernel is in class C or unpaired."""
import collections
import difflib
import re
import sys

RES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size",
       ".amdhsa_accum_offset")
LANE = ("v_writelane_b32", "v_readlane_b32")


def kernel_key(sym):
    """(base name, template arguments) of a mangled kernel symbol: _ZN12_GLOBAL__N_116emd_rows2_kernelILi4ELb1EEEv... ->
    ("emd_rows2_kernel", ("4", "true"))"""
    m = re.search(r"\d+(emd_\w+?_kernel)(I((?:L[a-z]\d+E)+)E)?", sym)
    if not m:
        return sym, ()
    args = []
    for t, v in re.findall(r"L([a-z])(\d+)E", m.group(3) or ""):
        args.append(("true" if v == "1" else "false") if t == "b" else v)
    return m.group(1), tuple(args)


def show(key):
    return key[0] + ("<" + ", ".join(key[1]) + ">" if key[1] else "")


def parse(path):
    """{key: {"text": [instruction lines], "res": {descriptor line: value}}} in file order"""
    lines = [l.split(";")[0].rstrip() for l in open(path).read().splitlines()]
    syms = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    out = collections.OrderedDict()
    for sym in syms:
        start = lines.index(sym + ":")
        text = []
        for l in lines[start + 1:]:
            s = l.strip()
            if s.startswith(".Lfunc_end"):
                break
            if not s or s.startswith(".") or s.endswith(":"):      # directives and labels
                continue
            text.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())))
        res = {}
        for l in lines[[x.strip() for x in lines].index(".amdhsa_kernel " + sym):]:
            p = l.split()
            if p and p[0] == ".end_amdhsa_kernel":
                break
            if p and p[0] in RES:
                res[p[0]] = p[1]
        out[kernel_key(sym)] = {"text": text, "res": res}
    return out


def reduced(text):
    out = []
    for l in text:
        m = l.split()[0]
        if (m.startswith("v_") and not m.startswith("v_mov")) or m.startswith(("ds_", "global_", "scratch_")) or m in (
                "s_barrier", "s_load_dwordx8", "s_load_dwordx16"):
            out.append(m)
    return out


def loop(seq):
    idx = [i for i, m in enumerate(seq) if m == "s_load_dwordx16"]
    return seq[idx[0]:idx[-1] + 1] if idx else None


def classify(a, b):
    """class, [reasons], loop diff lines"""
    if a["text"] == b["text"] and a["res"] == b["res"]:
        return "A", [], []
    why, diff = [], []
    ra, rb = reduced(a["text"]), reduced(b["text"])
    la, lb = loop(ra), loop(rb)
    if la != lb:
        why.append("(i) the loop's mnemonic sequence differs")
        diff = list(difflib.unified_diff(la or [], lb or [], "before", "after", lineterm="", n=2))
    ca, cb = collections.Counter(ra), collections.Counter(rb)
    for m in sorted(set(ca) | set(cb)):
        if ca[m] != cb[m] and not (m in LANE and cb[m] < ca[m]):
            why.append("(ii) %s: %d -> %d" % (m, ca[m], cb[m]))
    for r in RES:
        if a["res"].get(r) != b["res"].get(r):
            why.append("(iii) %s: %s -> %s" % (r, a["res"].get(r), b["res"].get(r)))
    return ("C" if why else "B"), why, diff


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    before, after = parse(sys.argv[1]), parse(sys.argv[2])
    left = dict(before)
    rows, details, bad = [], [], 0
    for key, kb in after.items():
        pk = key if key in left else next((k for k in left if k[0] == key[0] and k[1][:len(key[1])] == key[1] and k not in after), None)
        if pk is None:
            rows.append((show(key), "-", "unpaired", "", "", ""))
            bad += 1
            continue
        ka = left.pop(pk)
        cls, why, diff = classify(ka, kb)
        lanes = [sum(l.split()[0] in LANE for l in k["text"]) for k in (ka, kb)]
        note = "" if lanes[0] == lanes[1] else "lane writes + reads %d -> %d" % tuple(lanes)
        r = kb["res"]
        rows.append((show(key), show(pk) if pk != key else "", cls, "%d -> %d" % (len(ka["text"]), len(kb["text"])),
                     "%s / %s / %s / %s" % (r[RES[0]], r[RES[1]], r[RES[2]], r[RES[3]]), note))
        if cls == "C":
            bad += 1
            details.append((show(key), why, diff))
    for key in left:
        rows.append(("-", show(key), "unpaired", "", "", ""))
        bad += 1
    count = collections.Counter(r[2] for r in rows)
    print("%d kernels before, %d after: %s" % (len(before), len(after), ", ".join("%d in class %s" % (count[c], c) for c in sorted(count))))
    print()
    print("| kernel | paired with (before) | class | instructions | VGPR / SGPR / LDS / scratch (after) | |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| `%s` | %s | %s | %s | %s | %s |" % (r[0], "`%s`" % r[1] if r[1] else "", r[2], r[3], r[4], r[5]))
    for name, why, diff in details:
        print("\n### class C: `%s`\n" % name)
        for w in why:
            print("* " + w)
        if diff:
            print("\n```diff\n" + "\n".join(diff) + "\n```")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
