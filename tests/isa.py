"""What the static ISA tests share: tools/isa_stats.py loaded once, each source file cross-compiled to gfx950 assembly
once per process (composite.hip, the slowest, serves four test files), the float-atomic pattern and the opcode list."""
import functools
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
stats = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(stats)
stats.compile_isa = functools.lru_cache(maxsize=None)(stats.compile_isa)      # audit() compiles through this name too
audit = functools.lru_cache(maxsize=None)(stats.audit)                        # isa_stats.audit() of composite.hip

FLOAT_ATOMIC = re.compile(r"^\s*(\S*atomic_add_f\S*|\S*atomic_pk_add\S*|ds_add_f32|ds_add_rtn_f32|ds_pk_add_\S*)\b",
                          re.M)


@functools.lru_cache(maxsize=None)
def compiled(source):
  """(asm, kernels) of one file of csrc/: the assembly text and isa_stats.kernels() of it.  Shared: do not modify."""
  asm = stats.compile_isa(source)
  return asm, stats.kernels(asm)


def ops(body):
  """The first token of each instruction line of a kernel's body (comments, labels and directives left out)."""
  return [ln.split()[0] for ln in body if ln.strip() and not ln.strip().startswith((";", "."))]
