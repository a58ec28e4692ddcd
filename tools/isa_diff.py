#!/usr/bin/env python3
"""Do two csrc trees compile to the same device code?  (runs without a GPU)

    python tools/isa_diff.py BASE_CSRC NEW_CSRC [--out FILE.md]

For a change that is meant to leave every kernel alone.  Each *.hip of either directory is compiled with build.py's FLAGS (its -I
pointed at the tree in question) plus --cuda-device-only -S, at most four compilers at a time.  From the assembly go the .file and
.ident lines, comment-only lines and every line that names __hip_cuid_ (a hash of the source text); what is left is compared per
file.  One row per file: identical, or the first differing kernel and line.  Exit status 1 if any file differs."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "3d-point-clouds-autocomplete_amd"))
import build  # noqa: E402


def assembly(src):
    """the kept lines of src's device assembly, or the compiler's complaint as a string"""
    flags = [f for f in build.FLAGS if not f.startswith("-I")] + ["-I" + os.path.dirname(src)]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "a.s")
        r = subprocess.run([build.HIPCC] + flags + ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
        if r.returncode:
            return "does not compile: " + (r.stderr.strip().splitlines() or ["?"])[-1]
        keep = []
        for l in open(out):
            s = l.strip()
            if s.startswith((".file", ".ident", ";")) or "__hip_cuid_" in s:
                continue
            keep.append(l.rstrip())
        return keep


def first_difference(a, b):
    """(symbol, line number within it, base line, new line) of the first line at which a and b part"""
    sym, at = "(before the first symbol)", 0
    for i in range(max(len(a), len(b))):
        x, y = (a[i] if i < len(a) else "<end>"), (b[i] if i < len(b) else "<end>")
        if x != y:
            return sym, i - at, x.strip(), y.strip()
        m = re.match(r"([A-Za-z_$][\w$.]*):", x)      # a symbol's label (block labels start with a dot)
        if m:
            sym, at = m.group(1), i


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("base_csrc")
    ap.add_argument("new_csrc")
    ap.add_argument("--out", help="write the table to this file as well")
    args = ap.parse_args()
    trees = [os.path.abspath(args.base_csrc), os.path.abspath(args.new_csrc)]
    names = sorted({os.path.basename(p) for t in trees for p in glob.glob(os.path.join(t, "*.hip"))})
    jobs = [os.path.join(t, n) for n in names for t in trees]
    with ThreadPoolExecutor(max_workers=4) as ex:
        asm = list(ex.map(lambda p: assembly(p) if os.path.exists(p) else "missing", jobs))
    rows, bad = ["| file | lines | device code |", "|---|---|---|"], 0
    for k, n in enumerate(names):
        a, b = asm[2 * k], asm[2 * k + 1]
        if isinstance(a, str) or isinstance(b, str):
            bad += 1
            rows.append("| `%s` | | base: %s; new: %s |" % (n, a if isinstance(a, str) else "ok", b if isinstance(b, str) else "ok"))
        elif a == b:
            rows.append("| `%s` | %d | identical |" % (n, len(a)))
        else:
            bad += 1
            sym, line, x, y = first_difference(a, b)
            rows.append("| `%s` | %d / %d | differs in `%s`, line %d: `%s` -> `%s` |" % (n, len(a), len(b), sym, line, x, y))
    rows.append("")
    rows.append("%d files, %d identical, %d differ" % (len(names), len(names) - bad, bad))
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
