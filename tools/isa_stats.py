"""Static audit of the hot kernels' gfx950 code: registers, scratch, barriers, and the instruction mix of the
per-pair loop of K6 / K7 (packed fp32, plain VALU, transcendental, SALU, LDS, memory).

    python tools/isa_stats.py            # table
    python tools/isa_stats.py --json     # machine-readable (bench.py's VALU roofline leg and tests/test_isa_budget.py)

hipcc cross-compiles without a GPU, so this runs anywhere the toolchain is.  The per-instruction issue costs that turn
the mix into an issue-bound time are measured on the MI355X by tools/valu_rate.hip (profiles/r02_valu_issue_costs.txt).
"""
from __future__ import annotations

import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "splat-trainer_amd", "csrc")

TRANS = ("v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_sin_f32", "v_cos_f32")


def compile_isa(source: str = "composite.hip", csrc: str = CSRC) -> str:
  """gfx950 assembly of one source of `csrc` (this tree's csrc/, or the same directory of another checkout)."""
  hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  with tempfile.TemporaryDirectory() as tmp:
    out = os.path.join(tmp, "k.s")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                    "-Wno-unused-command-line-argument", "-o", out, source], check=True, cwd=csrc,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def classify(op: str) -> str:
  if op.startswith("v_pk_"):
    return "valu_packed"
  if op.startswith(TRANS):
    return "valu_trans"
  if op.startswith("v_"):
    return "valu"
  if op.startswith("ds_"):
    return "lds"
  if op.startswith(("s_load", "s_buffer_load")):
    return "smem"
  if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
    return "vmem"
  if op.startswith(("s_waitcnt", "s_nop")):
    return "wait"
  if op.startswith("s_"):
    return "salu"
  return "other"


def kernels(asm: str) -> dict:
  """name -> dict(vgpr, sgpr, scratch, lds, body=[instruction lines])."""
  meta = {}
  # one metadata entry per kernel: "  - .agpr_count: ..." up to the next entry; its own keys sit at four spaces (the keys
  # of its arguments deeper), in alphabetical order -- .group_segment_fixed_size in FRONT of .name
  for m in re.finditer(r"^  - (\.\w+:.*?)(?=^  - |^\S|\Z)", asm, flags=re.S | re.M):
    blk = "\n    " + m.group(1)
    mm = re.search(r"\n    \.name:\s+(\S+)", blk)
    if not mm:
      continue
    name = mm.group(1)
    def num(key):
      mm = re.search(rf"\n    \.{key}:\s+(\d+)", blk)
      return int(mm.group(1)) if mm else None
    if num("vgpr_count") is not None:
      meta[name] = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), scratch=num("private_segment_fixed_size"),
                        lds=num("group_segment_fixed_size"))
  for name in meta:
    m = re.search(rf"^{re.escape(name)}:.*?\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M)   # (a kernel may hold several s_endpgm)
    meta[name]["body"] = m.group(1).splitlines() if m else []
  return meta


def loop_mix(body, depth: int = 2) -> dict:
  """Instruction classes inside the deepest loop nest (lines tagged 'Depth=<depth>' by the compiler delimit the blocks:
  every basic block whose label comment says it belongs to that loop)."""
  mix, inside = {}, False
  for ln in body:
    s = ln.strip()
    if s.startswith(".LBB") or s.startswith("; %bb."):
      inside = f"Depth={depth}" in s or (inside and s.startswith("; %bb.") and "in Loop" in s and f"Depth={depth}" in s)
      if s.startswith(".LBB"):
        inside = f"Depth={depth}" in s
      continue
    if not inside or not s or s.startswith((";", ".")):
      continue
    op = s.split()[0]
    if op.startswith(";"):
      continue
    c = classify(op)
    mix[c] = mix.get(c, 0) + 1
  return mix


def blocks(body) -> list:
  """The kernel's basic blocks in layout order: dict(label, loop, header, lines) -- `loop` is the label of the header of
  the innermost loop the block belongs to (None outside every loop), from the compiler's block comments."""
  out = [dict(label="entry", loop=None, header=False, lines=[])]
  for ln in body:
    s = ln.strip()
    start = re.match(r"\.(LBB\d+_\d+):", s) or re.match(r"; %bb\.(\d+):", s)
    if start:
      out.append(dict(label=start.group(1).replace("LBB", "BB"), loop=None, header=False, lines=[]))
    if start or (s.startswith(";") and not out[-1]["lines"]):        # the block's own comment lines
      m = re.search(r"in Loop: Header=(BB\d+_\d+)", s)
      if m:
        out[-1]["loop"] = m.group(1)
      elif re.search(r"This (Inner )?Loop Header", s):
        out[-1]["loop"], out[-1]["header"] = out[-1]["label"], True
      continue
    if s and not s.startswith((";", ".")):
      out[-1]["lines"].append(s)
  return out


def is_vmcnt_wait(line: str) -> bool:
  return line.startswith("s_waitcnt") and "vmcnt" in line


def four_pair_loops(body) -> list:
  """K6: the innermost loops that hold the four-pair visibility reduction (v_permlane32_swap marks it), one per copy of
  the walk: dict(header, blocks, vmcnt_waits, vmem) -- waits on the vector-memory counter and vector-memory instructions
  inside the loop's own blocks."""
  bl = blocks(body)
  loops = []
  for b in bl:
    if b["loop"] and b["loop"] not in loops and any(l.startswith("v_permlane32_swap") for l in b["lines"]):
      loops.append(b["loop"])
  out = []
  for h in loops:
    mine = [b for b in bl if b["loop"] == h]
    out.append(dict(header=h, blocks=len(mine),
                    vmcnt_waits=sum(1 for b in mine for l in b["lines"] if is_vmcnt_wait(l)),
                    vmem=sum(1 for b in mine for l in b["lines"] if classify(l.split()[0]) == "vmem")))
  return out


def prologue_vmcnt_waits(body) -> int:
  """K7: waits on the vector-memory counter from the kernel's entry to its first loop (the chunk loop)."""
  n = 0
  for b in blocks(body):
    if b["header"]:
      return n
    n += sum(1 for l in b["lines"] if is_vmcnt_wait(l))
  raise ValueError("no loop in the kernel")


def waits_to_first_store(body) -> dict:
  """The per-splat and sort kernels: memory round trips from the kernel's entry to its first global store, in layout
  order.  A wait counts as a trip when at least one load of its kind went out since the last counted one (several partial
  waits on one batch of loads are one trip): dict(vmem_waits, smem_waits, vmem_loads) -- vector loads before the store."""
  vm = sm = loads = 0
  vm_open = sm_open = False
  for ln in body:
    s = ln.strip()
    if not s or s.startswith((";", ".")):
      continue
    op = s.split()[0]
    if op.startswith(("global_store", "buffer_store", "flat_store")):
      return dict(vmem_waits=vm, smem_waits=sm, vmem_loads=loads)
    c = classify(op)
    if c == "vmem" and "_load" in op:
      vm_open, loads = True, loads + 1
    elif c == "smem":
      sm_open = True
    elif op == "s_waitcnt":
      if "vmcnt" in s and vm_open:
        vm, vm_open = vm + 1, False
      if "lgkmcnt" in s and sm_open:
        sm, sm_open = sm + 1, False
  raise ValueError("no global store in the kernel")


# the kernels of a frame whose loads go out when their address is known (tests/test_isa_budget_frame_waits.py):
# label -> (source file, needles of the mangled name)
FRAME_WAIT_KERNELS = {
    "cull_count": ("geometry.hip", ("cull_count_kernel",)),
    "cull_write": ("geometry.hip", ("cull_write_kernel",)),
    "project_sh_fwd_K16": ("geometry.hip", ("project_sh_fwd_kernelILi16ELb1E",)),
    "project_sh_fwd_K9": ("geometry.hip", ("project_sh_fwd_kernelILi9ELb1E",)),
    "project_sh_fwd_K9_nojac": ("geometry.hip", ("project_sh_fwd_kernelILi9ELb0E",)),
    "project_sh_fwd_K4": ("geometry.hip", ("project_sh_fwd_kernelILi4ELb1E",)),
    "project_sh_fwd_K1": ("geometry.hip", ("project_sh_fwd_kernelILi1ELb1E",)),
    "rs_hist_9": ("prims.hip", ("rs_hist_kernelILi9E",)),
    "rs_hist_8": ("prims.hip", ("rs_hist_kernelILi8E",)),
    "rs_scatter_1v_4_9": ("prims.hip", ("rs_scatter_kernelILb0ELi4ELi9E",)),
    "rs_scatter_1v_4_8": ("prims.hip", ("rs_scatter_kernelILb0ELi4ELi8E",)),
    "rs_scatter_2v_4_8": ("prims.hip", ("rs_scatter_kernelILb1ELi4ELi8E",)),
    "rs_scatter_2v_16_8": ("prims.hip", ("rs_scatter_kernelILb1ELi16ELi8E",)),
    "tile_count": ("binning.hip", ("tile_count_kernel",)),
    "reduce_grad": ("binning.hip", ("18reduce_grad_kernel",)),
}


def frame_waits() -> dict:
  out = {}
  for label, (source, needles) in FRAME_WAIT_KERNELS.items():
    meta = kernels(compile_isa(source))
    k = meta[find(meta, *needles)]
    out[label] = dict(waits_to_first_store(k["body"]), vgpr=k["vgpr"], sgpr=k["sgpr"], lds_bytes=k["lds"],
                      scratch_bytes=k["scratch"])
  return out


def find(meta: dict, *needles: str) -> str:
  for name in meta:
    if all(n in name for n in needles):
      return name
  raise KeyError(needles)


def audit() -> dict:
  meta = kernels(compile_isa("composite.hip"))
  out = {}
  picks = {"K7_bwd_C3": ("composite_bwd_kernelILi3E",), "K6_fwd_C3_vis": ("composite_fwd_kernelILi3ELb1ELb0ELb0E",),
           "K6_fwd_C3_vis_prefetch": ("composite_fwd_kernelILi3ELb1ELb0ELb1E",),
           "K6_segC_C3_vis": ("seg_composite_kernelILi3ELb1ELb0ELb0E",), "K6_combine_C3": ("seg_combine_kernelILi3ELb0E",)}
  for label, needles in picks.items():
    k = meta[find(meta, *needles)]
    body = k["body"]
    depth = 2 if any("Depth=2" in ln for ln in body) else 1
    out[label] = dict(vgpr=k["vgpr"], sgpr=k["sgpr"], scratch_bytes=k["scratch"], lds_bytes=k["lds"],
                      s_barrier=sum(1 for ln in body if ln.strip().startswith("s_barrier")),
                      mfma=sum(1 for ln in body if "mfma" in ln), static_loop_mix=loop_mix(body, depth),
                      instructions=sum(1 for ln in body if ln.strip() and not ln.strip().startswith((";", "."))))
  # where the composite walks wait for memory (tests/test_isa_budget_composite_waits.py)
  out["composite_waits"] = {
      "K6_fwd_C3_vis": dict(four_pair_loops=four_pair_loops(meta[find(meta, *picks["K6_fwd_C3_vis"])]["body"])),
      "K6_segC_C3_vis": dict(four_pair_loops=four_pair_loops(meta[find(meta, *picks["K6_segC_C3_vis"])]["body"])),
      "K7_bwd_C3": dict(prologue_vmcnt_waits=prologue_vmcnt_waits(meta[find(meta, *picks["K7_bwd_C3"])]["body"]))}
  # where the per-splat and sort kernels of a frame wait for memory (tests/test_isa_budget_frame_waits.py)
  out["frame_waits"] = frame_waits()
  out["all_kernels"] = {n: dict(vgpr=k["vgpr"], scratch_bytes=k["scratch"]) for n, k in meta.items()}
  return out


if __name__ == "__main__":
  a = audit()
  if "--json" in sys.argv:
    print(json.dumps(a))
  else:
    for label, k in a.items():
      if label in ("all_kernels", "composite_waits", "frame_waits"):
        continue
      print(f"{label:18s} vgpr {k['vgpr']:3d}  sgpr {k['sgpr']:3d}  scratch {k['scratch_bytes']} B  lds {k['lds_bytes']} B  "
            f"s_barrier {k['s_barrier']}  mfma {k['mfma']}  loop mix {k['static_loop_mix']}")
    for label, w in a["composite_waits"].items():
      print(f"{label:18s} waits {w}")
    for label, w in a["frame_waits"].items():
      print(f"{label:18s} to first store: vmem waits {w['vmem_waits']} ({w['vmem_loads']} loads)  smem waits {w['smem_waits']}  "
            f"vgpr {w['vgpr']}  sgpr {w['sgpr']}  lds {w['lds_bytes']} B  scratch {w['scratch_bytes']} B")
    worst = max(a["all_kernels"].values(), key=lambda k: k["scratch_bytes"])
    print(f"{len(a['all_kernels'])} kernels in composite.hip; max scratch {worst['scratch_bytes']} B")
