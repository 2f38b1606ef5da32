#!/usr/bin/env python3
"""Compare the gfx950 assembly of every csrc/hip/*.hip between a git revision and the working tree.

    python tools/isa_diff.py REV

Each file is compiled twice with the flags tools/build.py uses (device only,
-S): once as of REV (with REV's headers, from `git archive`), once from the
working tree.  Lines containing __hip_cuid_ (a per-compile hash) are dropped;
the rest is compared as text.  Prints `identical` per file, or the first
differing kernel symbol and the number of differing lines; exit status 1 if
any file differs.  A refactor that must not change device code passes when
every file is identical.
"""
import concurrent.futures as cf
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.build import HIPCC, hip_flags  # noqa: E402


def asm(src):
    """Device assembly lines of `src`; None where the file does not exist."""
    if not os.path.exists(src):
        return None
    cmd = [HIPCC] + hip_flags(os.path.basename(src)) + ["--cuda-device-only", "-S", "-o", "-", src]
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
    return [l for l in out.split("\n") if "__hip_cuid_" not in l]


def compare(old, new):
    if old is None or new is None:
        return "only in " + ("the working tree" if old is None else "REV")
    if old == new:
        return "identical"
    first = next((i for i, (a, b) in enumerate(zip(old, new)) if a != b), min(len(old), len(new)))
    tail = next((i for i, (a, b) in enumerate(zip(old[:first:-1], new[:first:-1])) if a != b), 0)
    mid_old, mid_new = old[first:len(old) - tail], new[first:len(new) - tail]  # the diff runs on the middle only
    n = sum(max(i1 - i0, j1 - j0) for tag, i0, i1, j0, j1 in
            difflib.SequenceMatcher(None, mid_old, mid_new, autojunk=False).get_opcodes() if tag != "equal")
    sym = "(file prologue)"
    for l in new[:first + 1]:
        m = re.match(r"(_Z\w+):", l)
        if m:
            sym = m.group(1)
    return f"DIFFERS: first in {sym}, {n} lines"


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    with tempfile.TemporaryDirectory() as td:
        ar = subprocess.run(["git", "-C", ROOT, "archive", sys.argv[1], "csrc/hip"], check=True, stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", td], input=ar.stdout, check=True)
        names = sorted({os.path.basename(p) for d in (ROOT, td) for p in glob.glob(os.path.join(d, "csrc", "hip", "*.hip"))})
        with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
            olds = list(ex.map(asm, [os.path.join(td, "csrc", "hip", n) for n in names]))
            news = list(ex.map(asm, [os.path.join(ROOT, "csrc", "hip", n) for n in names]))
    bad = 0
    for n, o, w in zip(names, olds, news):
        res = compare(o, w)
        bad += res != "identical"
        print(f"{n:16s} {res}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
