#!/usr/bin/env python3
"""One line per gfx950 kernel in the objects of a build directory: what the device code IS, for comparing two builds.

    python tools/device_code_digest.py vdn-nerf_amd/vdn_hip/_build > listing.txt

Per kernel symbol: object, symbol, size in bytes, sha256 of its bytes in .text, and from the code object's kernel notes the
VGPR / AGPR / SGPR counts, the LDS (group segment) and scratch (private segment) sizes and the spill counts. Two builds whose
listings are equal run the same instructions with the same resources. It looks for nothing: it only hashes and lists.
Needs llvm-objdump and llvm-readelf (ROCm's LLVM); no GPU, no torch.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
NOTES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
         "vgpr_spill_count", "sgpr_spill_count")


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, capture_output=True, text=True, cwd=cwd).stdout


def kernels(code_object):
    """[(symbol, size, sha256 of its .text bytes, the NOTES values)] of one code object, sorted by symbol."""
    sec = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run("llvm-readelf", "-S", "-W", code_object))
    if sec is None:
        return []
    addr, off = int(sec.group(1), 16), int(sec.group(2), 16)
    blob = open(code_object, "rb").read()
    notes = {}          # kernel name -> its notes (the metadata lists each kernel as a block of ".key: value" lines)
    for block in re.split(r"\n  - ", run("llvm-readelf", "--notes", code_object))[1:]:
        kv = dict(re.findall(r"^ {4}\.(\w+): +'?([^'\n]+)'?$", "    " + block, re.M))          # (deeper lines are its arguments)
        if "name" in kv and "symbol" in kv:
            notes[kv["name"]] = kv
    out = set()         # (a symbol is listed in .dynsym and in .symtab)
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\w+\s+\w+\s+\d+\s+(\S+)$", run("llvm-readelf", "-s", "-W", code_object), re.M):
        value, size, name = int(m.group(1), 16), int(m.group(2)), m.group(3)
        if name in notes:
            start = value - addr + off
            out.add((name, size, hashlib.sha256(blob[start:start + size]).hexdigest(), tuple(notes[name].get(k, "-") for k in NOTES)))
    return sorted(out)


def main(objdir):
    for obj in sorted(f for f in os.listdir(objdir) if f.endswith(".o")):
        with tempfile.TemporaryDirectory() as tmp:
            local = os.path.join(tmp, obj)
            os.symlink(os.path.abspath(os.path.join(objdir, obj)), local)
            run("llvm-objdump", "--offloading", local, cwd=tmp)         # writes <obj>.<n>.hip-amdgcn-amd-amdhsa--gfx950 next to it
            for co in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
                for name, size, digest, vals in kernels(os.path.join(tmp, co)):
                    print(obj, name, size, digest, " ".join("%s=%s" % kv for kv in zip(NOTES, vals)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
