#!/usr/bin/env python3
"""Criteo-style TSV click log → a click directory for ``--workload wide_deep / deepfm --data``.

    python tools/criteo_to_clicks.py train.txt clicks/train
    python tools/criteo_to_clicks.py valid.txt clicks/valid --stats-from clicks/train

A line is ``label \\t I1 … I13 \\t C1 … C26``: a 0 / 1 label, 13 integer features and 26
categorical tokens of up to 8 hex digits; an empty field is a missing value.  The directory
written is the format of ``paddle_operator_amd.data.CLICK_DOC``:

* ``cat.npy``    uint32 ``[n, 26]`` — the token as a number, 0 where it is missing;
* ``dense.npy``  int32 ``[n, 13]`` — the integer, −2³¹ where it is missing;
* ``label.npy``  uint8 ``[n]``;
* ``dense_stats.npy`` float32 ``[2, 13]`` — per feature the minimum of the present values and
  max − min (1 where that is 0, or where no value is present), the min–max rule of Paddle's
  Criteo readers.  ``--stats-from DIR`` copies DIR's file instead: a validation split is
  normalised with the training split's statistics.

Two streaming passes (count the lines, then fill the memory-mapped arrays a chunk at a time):
the log is never held in memory.
"""
import argparse
import os
import shutil
import sys

import numpy as np

MISSING = -(1 << 31)


def convert(src: str, out: str, n_dense: int = 13, n_sparse: int = 26, stats_from: str | None = None,
            chunk: int = 1 << 16) -> int:
    """Write the click directory ``out`` from the TSV ``src``; returns the number of records."""
    with open(src) as f:
        n = sum(1 for line in f if line.strip())
    if not 1 <= n < 1 << 31:
        raise SystemExit(f"{src}: {n} records, 1 <= n < 2^31 required")
    os.makedirs(out, exist_ok=True)
    mm = np.lib.format.open_memmap
    cat = mm(os.path.join(out, "cat.npy"), mode="w+", dtype=np.uint32, shape=(n, n_sparse))
    dense = mm(os.path.join(out, "dense.npy"), mode="w+", dtype=np.int32, shape=(n, n_dense))
    label = mm(os.path.join(out, "label.npy"), mode="w+", dtype=np.uint8, shape=(n,))
    lo = np.full(n_dense, np.iinfo(np.int64).max, dtype=np.int64)
    hi = np.full(n_dense, np.iinfo(np.int64).min, dtype=np.int64)
    width = 1 + n_dense + n_sparse

    def flush(at, rows):
        c = np.array([r[2] for r in rows], dtype=np.uint32).reshape(len(rows), n_sparse)
        d = np.array([r[1] for r in rows], dtype=np.int64).reshape(len(rows), n_dense)
        cat[at:at + len(rows)] = c
        dense[at:at + len(rows)] = d.astype(np.int32)
        label[at:at + len(rows)] = np.array([r[0] for r in rows], dtype=np.uint8)
        present = d != MISSING
        np.minimum(lo, np.where(present, d, np.iinfo(np.int64).max).min(axis=0), out=lo)
        np.maximum(hi, np.where(present, d, np.iinfo(np.int64).min).max(axis=0), out=hi)

    at, rows = 0, []
    with open(src) as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            fields = line.rstrip("\r\n").split("\t")
            if len(fields) != width:
                raise SystemExit(f"{src}:{no}: {len(fields)} fields, {width} expected")
            if fields[0] not in ("0", "1"):
                raise SystemExit(f"{src}:{no}: label {fields[0]!r}, 0 or 1 expected")
            try:
                d = [int(x) if x else MISSING for x in fields[1:1 + n_dense]]
                c = [int(x, 16) if x else 0 for x in fields[1 + n_dense:]]
            except ValueError as e:
                raise SystemExit(f"{src}:{no}: {e}")
            if any(x and not MISSING < v < 1 << 31 for x, v in zip(fields[1:1 + n_dense], d)):
                raise SystemExit(f"{src}:{no}: an integer feature outside (-2^31, 2^31)")
            if any(v >> 32 for v in c):
                raise SystemExit(f"{src}:{no}: a categorical token of more than 8 hex digits")
            rows.append((int(fields[0]), d, c))
            if len(rows) == chunk:
                flush(at, rows)
                at, rows = at + len(rows), []
    if rows:
        flush(at, rows)
    for a in (cat, dense, label):
        a.flush()
    dst = os.path.join(out, "dense_stats.npy")
    if stats_from:
        shutil.copyfile(os.path.join(stats_from, "dense_stats.npy"), dst)
    else:
        seen = hi >= lo
        mn = np.where(seen, lo, 0)
        diff = np.where(seen, hi - lo, 1)
        np.save(dst, np.stack([mn, np.where(diff == 0, 1, diff)]).astype(np.float32))
    return n


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src", help="Criteo-style TSV")
    ap.add_argument("out", help="click directory to write")
    ap.add_argument("--stats-from", default="", help="copy this click directory's dense_stats.npy")
    ap.add_argument("--n-dense", type=int, default=13)
    ap.add_argument("--n-sparse", type=int, default=26)
    ap.add_argument("--chunk", type=int, default=1 << 16, help="lines parsed per write")
    a = ap.parse_args(argv)
    n = convert(a.src, a.out, a.n_dense, a.n_sparse, a.stats_from or None, a.chunk)
    print(f"{a.out}: {n} records", file=sys.stderr)


if __name__ == "__main__":
    main()
