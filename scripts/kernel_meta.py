"""Register / spill / LDS figures of the gfx950 kernels inside libbm_gar.so (no GPU needed).

    python scripts/kernel_meta.py [regex on the demangled kernel name]
    python scripts/kernel_meta.py diff LIB_A LIB_B      the proof that a host-only change left the device code alone

Extracts the code objects with llvm-objdump --offloading into a temporary directory and reads the
AMDGPU metadata notes (llvm-readelf --notes)."""
import hashlib
import pathlib
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = pathlib.Path("/opt/rocm/lib/llvm/bin")
LIB = pathlib.Path(__file__).resolve().parent.parent / "byzantinemomentum_amd" / "libbm_gar.so"


def kernels(lib=LIB):
  out = []
  with tempfile.TemporaryDirectory() as tmp:
    local = pathlib.Path(tmp) / lib.name
    shutil.copy(lib, local)
    subprocess.run([LLVM / "llvm-objdump", "--offloading", local], cwd=tmp, capture_output=True, check=True)
    for co in sorted(pathlib.Path(tmp).glob("*gfx950*")):
      notes = subprocess.run([LLVM / "llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
      for block in notes.split("  - .agpr_count:")[1:]:
        def field(name, cast=int):
          m = re.search(r"\." + name + r":\s+(\S+)", block)
          return cast(m.group(1)) if m else None
        out.append({"name": field("name", str), "vgpr": field("vgpr_count"), "sgpr": field("sgpr_count"),
                    "sgpr_spill": field("sgpr_spill_count"), "vgpr_spill": field("vgpr_spill_count"),
                    "lds": field("group_segment_fixed_size"), "scratch": field("private_segment_fixed_size")})
  names = subprocess.run(["c++filt"], input="\n".join(k["name"] for k in out), capture_output=True, text=True).stdout.split("\n")
  for k, nm in zip(out, names):
    k["demangled"] = nm
  return out


def packed_fp32(lib=LIB):
  """{kernel symbol: number of v_pk_{add,mul,fma}_f32 instructions} over the gfx950 code objects of the library — must
  be empty (byzantinemomentum_amd/build.py: the packed forms gave wrong results under GPU sharing)."""
  found = {}
  with tempfile.TemporaryDirectory() as tmp:
    local = pathlib.Path(tmp) / lib.name
    shutil.copy(lib, local)
    subprocess.run([LLVM / "llvm-objdump", "--offloading", local], cwd=tmp, capture_output=True, check=True)
    for co in sorted(pathlib.Path(tmp).glob("*gfx950*")):
      text = subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
      name = None
      for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
          name = m.group(1)
        elif re.search(r"\bv_pk_(add|mul|fma)_f32\b", line):
          found[name] = found.get(name, 0) + 1
  return found


def isa_hashes(lib=LIB):
  """{kernel symbol: sha256 of its disassembled instruction text} over the gfx950 code objects of the library (a kernel
  that several translation units hold, such as eval_finish_kernel, is keyed "symbol @ code object number")."""
  text = {}
  with tempfile.TemporaryDirectory() as tmp:
    local = pathlib.Path(tmp) / pathlib.Path(lib).name
    shutil.copy(lib, local)
    subprocess.run([LLVM / "llvm-objdump", "--offloading", local], cwd=tmp, capture_output=True, check=True)
    for number, co in enumerate(sorted(pathlib.Path(tmp).glob("*gfx950*"))):
      dis = subprocess.run([LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                           capture_output=True, text=True, check=True).stdout
      name = None
      for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if m:
          name = m.group(1) if m.group(1) not in text else f"{m.group(1)} @ {number}"
          text[name] = []
        elif name is not None and line.strip():
          text[name].append(line.split("//")[0].strip())  # (the comment holds the address: where the kernel lies, not what it is)
  return {k: hashlib.sha256("\n".join(v).encode()).hexdigest() for k, v in text.items()}


def diff(lib_a, lib_b):
  """Prints the kernel symbols only one library has and those whose instructions differ; returns their number."""
  a, b = isa_hashes(lib_a), isa_hashes(lib_b)
  only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
  changed = sorted(k for k in set(a) & set(b) if a[k] != b[k])
  for title, names in (("only in A", only_a), ("only in B", only_b), ("instructions differ", changed)):
    for nm in names:
      print(f"{title}: {nm}")
  print(f"A: {len(a)} kernel symbols, B: {len(b)}; only in A {len(only_a)}, only in B {len(only_b)}, "
        f"instructions differ {len(changed)}")
  return len(only_a) + len(only_b) + len(changed)


if __name__ == "__main__":
  if len(sys.argv) == 4 and sys.argv[1] == "diff":
    sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
  pat = re.compile(sys.argv[1]) if len(sys.argv) > 1 else None
  print(f"{'vgpr':>5} {'sgpr':>5} {'s_spill':>7} {'v_spill':>7} {'lds':>7} {'scratch':>7}  kernel")
  for k in kernels():
    if pat is None or pat.search(k["demangled"]):
      print(f"{k['vgpr']:>5} {k['sgpr']:>5} {k['sgpr_spill']:>7} {k['vgpr_spill']:>7} {k['lds']:>7} {k['scratch']:>7}  {k['demangled'][:150]}")
