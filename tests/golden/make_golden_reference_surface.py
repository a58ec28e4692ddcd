#!/usr/bin/env python3
"""Generate tests/golden/reference_surface.npz from a checkout of the reference project (CPU only):

    python tests/golden/make_golden_reference_surface.py <reference-tree>

The fixture holds data about the reference's Python files, none of their text:
  lines/<rel path>      one 64-bit hash (first 8 bytes of SHA-256) per code line of every reference .py file, lines
                        normalised as tools/line_overlap.py does (comments, blank lines and docstring quotes dropped,
                        whitespace collapsed) — what tests/test_capi_symbols.py measures the same-named files here against
  loop_imports          "module:name" for every `from module import name` of core/epoch_loops.py
  loop_forward_arity    number of positional arguments each of its calls of the model passes (train_epoch, val_epoch)
  loop_model_attrs      attribute chains it reads off the model argument (e.g. "mode.has_generativity")
The last three are what tests/test_host_logic.py binds this package's modules against.
"""
import ast
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_surface.npz")


def _line_overlap():
    spec = importlib.util.spec_from_file_location("line_overlap", os.path.join(ROOT, "tools", "line_overlap.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def line_hash(line):
    return int.from_bytes(hashlib.sha256(line.encode("utf-8")).digest()[:8], "little")


def _attr_chain(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    return (node.id if isinstance(node, ast.Name) else None), ".".join(reversed(parts))


def loop_surface(path):
    tree = ast.parse(open(path, encoding="utf-8").read())
    imports = sorted({f"{n.module}:{a.name}" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) for a in n.names})
    arity, attrs = [], set()
    for fn in tree.body:
        if not isinstance(fn, ast.FunctionDef):
            continue
        model = fn.args.args[1].arg                      # train_epoch(epoch, full_model, ...), val_epoch(epoch, full_model, ...)
        for n in ast.walk(fn):
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == model:
                arity.append(len(n.args))
            if isinstance(n, ast.Attribute):
                base, chain = _attr_chain(n)
                if base == model:
                    attrs.add(chain)
    # keep the longest chain only ("mode.has_generativity" covers "mode")
    attrs = sorted(a for a in attrs if not any(b != a and b.startswith(a + ".") for b in attrs))
    return imports, arity, attrs


def main(ref):
    lo = _line_overlap()
    arrays = {}
    for root, _, files in os.walk(ref):
        for f in sorted(files):
            if f.endswith(".py"):
                path = os.path.join(root, f)
                rel = os.path.relpath(path, ref)
                arrays["lines/" + rel] = np.array([line_hash(ln) for ln in lo.code_lines(path)], dtype=np.uint64)
    imports, arity, attrs = loop_surface(os.path.join(ref, "core", "epoch_loops.py"))
    arrays["loop_imports"] = np.array(imports)
    arrays["loop_forward_arity"] = np.array(arity, dtype=np.int64)
    arrays["loop_model_attrs"] = np.array(attrs)
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, "-", sum(k.startswith("lines/") for k in arrays), "files;", imports, arity, attrs)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
