"""Proves that a change left the device code alone: the gfx950 code of every HIP source, compared kernel by kernel
between a revision and the working tree.

    python tools/device_code_diff.py REV            # e.g. HEAD, main, a commit id

Each source of build.HIP_SOURCES is cross-compiled to assembly twice (tools/isa_stats.py: compile_isa, no GPU needed):
from REV's tree, exported with `git archive` into a temporary directory, and from the working tree.  Per kernel
(isa_stats.kernels) it compares the name, the body -- every instruction, label and directive between the kernel's label
and its end, without the comments and with the function-index part of local labels taken out, since only the order of
the kernels in the file may change -- and VGPRs, SGPRs, scratch and LDS bytes.  Prints one line per source (kernels
compared; the names that differ, appear or vanish) and exits 1 when any does.
"""
from __future__ import annotations

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


def export_tree(rev: str, into: str) -> str:
  """REV's include/ and csrc/ under `into`; returns its csrc directory."""
  tar = subprocess.run(["git", "archive", rev, "include", f"{PKG}/csrc"], cwd=ROOT, check=True, capture_output=True).stdout
  tarfile.open(fileobj=io.BytesIO(tar)).extractall(into)
  return os.path.join(into, PKG, "csrc")


def compare(source: str, old_csrc: str) -> dict:
  old = isa_stats.kernels(isa_stats.compile_isa(source, old_csrc))
  new = isa_stats.kernels(isa_stats.compile_isa(source))
  differ = []
  for name in sorted(set(old) & set(new)):
    o, n = old[name], new[name]
    what = [k for k in ("vgpr", "sgpr", "scratch", "lds") if o[k] != n[k]]
    if normalised(o["body"]) != normalised(n["body"]):
      what.append("body")
    if what:
      differ.append(f"{name} ({', '.join(what)})")
  return dict(compared=len(set(old) & set(new)), differ=differ, appear=sorted(set(new) - set(old)),
              vanish=sorted(set(old) - set(new)))


def main(rev: str) -> int:
  bad = total = 0
  with tempfile.TemporaryDirectory() as tmp:
    old_csrc = export_tree(rev, tmp)
    jobs = min(8, os.cpu_count() or 1)
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
      results = list(pool.map(lambda s: compare(s, old_csrc), build.HIP_SOURCES))
  for source, r in zip(build.HIP_SOURCES, results):
    total += r["compared"]
    print(f"{source:18s} {r['compared']:4d} kernels compared, {len(r['differ'])} differ, {len(r['appear'])} appear, "
          f"{len(r['vanish'])} vanish")
    for kind in ("differ", "appear", "vanish"):
      for name in r[kind]:
        bad += 1
        print(f"    {kind}: {name}")
  print(f"{len(results)} sources, {total} kernels compared against {rev}: "
        + ("device code identical" if not bad else f"{bad} kernels differ, appear or vanish"))
  return 1 if bad else 0


if __name__ == "__main__":
  if len(sys.argv) != 2:
    sys.exit(__doc__)
  sys.exit(main(sys.argv[1]))
