"""The evaluation's file protocol (core/experiments.py `fixed()` writes it; utils/evaluation/*.py `process()` reads it):
``<cat>_<i>_<j>_reconstruction.npy`` (3, N) for the k = 10 completions j of input i and ``<cat>_<i>_existing.npy``
(3, Ne) for the partial input itself, all in one directory.

Grouping follows the reference exactly: the reconstructions are taken in lexicographic ``sorted(glob)`` order and cut
into consecutive groups of 10, and the i-th existing file in the same order is the input of group i.  Because each name
ends in ``_<i>_`` both lists sort the inputs alike (``car_10_`` before ``car_1_``).  Unlike the reference, counts that
do not fit that protocol are an error rather than silently truncated.
"""
import glob
import os

import numpy as np

GROUP = 10


def reconstruction_paths(shape_dir):
    return sorted(glob.glob(os.path.join(shape_dir, "*reconstruction.npy")))


def existing_paths(shape_dir):
    return sorted(glob.glob(os.path.join(shape_dir, "*existing.npy")))


def grouped_paths(shape_dir, with_existing):
    """([S][10] reconstruction paths, [S] existing paths or None)."""
    rec = reconstruction_paths(shape_dir)
    if not rec or len(rec) % GROUP:
        raise ValueError(f"{shape_dir}: {len(rec)} reconstruction files, expected a positive multiple of {GROUP}")
    groups = [rec[i:i + GROUP] for i in range(0, len(rec), GROUP)]
    if not with_existing:
        return groups, None
    ex = existing_paths(shape_dir)
    if len(ex) != len(groups):
        raise ValueError(f"{shape_dir}: {len(ex)} existing files for {len(groups)} groups of {GROUP} reconstructions")
    return groups, ex


def load_points(paths):
    """Stack (3, N) files as one (len, N, 3) fp32 array."""
    return np.ascontiguousarray(np.stack([np.load(p).T for p in paths], axis=0), dtype=np.float32)
