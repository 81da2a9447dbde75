"""Proves that a change left the device code alone: the gfx950 code of every HIP source, compared kernel by kernel
between a revision and the working tree.

    python tools/device_code_diff.py REV            # e.g. HEAD, main, a commit id

Each source of build.HIP_SOURCES is cross-compiled to assembly twice (tools/isa_stats.py: compile_isa, no GPU needed):
from REV's tree, exported with `git archive` into a temporary directory, and from the working tree.  Per kernel
(isa_stats.kernels) it compares the name, the body -- every instruction, label and directive between the kernel's label
and its end, without the comments and with the function-index part of local labels taken out, since only the order of
the kernels in the file may change -- and VGPRs, SGPRs, scratch and LDS bytes.  Prints one line per source (kernels
compared; the names that differ, appear or vanish) and exits 1 when any does.

A kernel that is not identical is `reordered` when it executes the same instructions in another order or on other
registers: the same multiset of mnemonics, VGPRs and scratch not above REV's, LDS bytes equal.  That is proof of
unchanged behaviour only where the change touched integer arithmetic alone (integer sums are exact in any order); it is
reported beside `differ`, does not fail the run, and is for the reader to hold against what the change touched.
"""
from __future__ import annotations

import collections
import concurrent.futures
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "splat-trainer_amd"
sys.path.insert(0, os.path.join(ROOT, PKG))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build       # noqa: E402
import isa_stats   # noqa: E402

# .LBB<function>_<block>, .Lfunc_begin<function>, .Lfunc_end<function>, .LJTI<function>_<table>, ...: the compiler
# numbers a translation unit's functions in the order it emits them
_LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+(_\d+)?\b")


def normalised(body) -> list:
  """The body's instructions, labels and directives: comments (they name blocks by function index too) and the blank
  lines they leave are dropped, local labels lose their function index."""
  lines = (ln.split(";", 1)[0].rstrip() for ln in body)
  return [_LOCAL_LABEL.sub(lambda m: f".L{m.group(1)}{m.group(2) or ''}", ln) for ln in lines if ln]


def mnemonics(body) -> collections.Counter:
  """How often each instruction occurs in the body, operands aside (labels and directives are not instructions)."""
  return collections.Counter(ln.split()[0] for ln in normalised(body) if not ln.lstrip().startswith(".") and not ln.endswith(":"))


def export_tree(rev: str, into: str) -> str:
  """REV's include/ and csrc/ under `into`; returns its csrc directory."""
  tar = subprocess.run(["git", "archive", rev, "include", f"{PKG}/csrc"], cwd=ROOT, check=True, capture_output=True).stdout
  tarfile.open(fileobj=io.BytesIO(tar)).extractall(into)
  return os.path.join(into, PKG, "csrc")


def classify(old: dict, new: dict) -> dict:
  """Two isa_stats.kernels tables of one source -> compared (count) and the names that differ, are reordered, appear and
  vanish."""
  differ, reordered = [], []
  for name in sorted(set(old) & set(new)):
    o, n = old[name], new[name]
    what = [k for k in ("vgpr", "sgpr", "scratch", "lds") if o[k] != n[k]]
    if normalised(o["body"]) != normalised(n["body"]):
      what.append("body")
    if not what:
      continue
    same_work = (mnemonics(o["body"]) == mnemonics(n["body"]) and n["vgpr"] <= o["vgpr"] and n["scratch"] <= o["scratch"]
                 and n["lds"] == o["lds"])
    (reordered if same_work else differ).append(f"{name} ({', '.join(what)})")
  return dict(compared=len(set(old) & set(new)), differ=differ, reordered=reordered, appear=sorted(set(new) - set(old)),
              vanish=sorted(set(old) - set(new)))


def compare(source: str, old_csrc: str) -> dict:
  return classify(isa_stats.kernels(isa_stats.compile_isa(source, old_csrc)), isa_stats.kernels(isa_stats.compile_isa(source)))


def main(rev: str) -> int:
  bad = moved = total = 0
  with tempfile.TemporaryDirectory() as tmp:
    old_csrc = export_tree(rev, tmp)
    jobs = min(8, os.cpu_count() or 1)
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
      results = list(pool.map(lambda s: compare(s, old_csrc), build.HIP_SOURCES))
  for source, r in zip(build.HIP_SOURCES, results):
    total += r["compared"]
    moved += len(r["reordered"])
    print(f"{source:18s} {r['compared']:4d} kernels compared, {len(r['differ'])} differ, {len(r['reordered'])} reordered, "
          f"{len(r['appear'])} appear, {len(r['vanish'])} vanish")
    for kind in ("differ", "reordered", "appear", "vanish"):
      for name in r[kind]:
        bad += kind != "reordered"
        print(f"    {kind}: {name}")
  verdict = "device code identical" if not bad else f"{bad} kernels differ, appear or vanish"
  print(f"{len(results)} sources, {total} kernels compared against {rev}: {verdict}"
        + (f"; {moved} reordered (same instructions, registers and LDS within REV's)" if moved else ""))
  return 1 if bad else 0


if __name__ == "__main__":
  if len(sys.argv) != 2:
    sys.exit(__doc__)
  sys.exit(main(sys.argv[1]))
