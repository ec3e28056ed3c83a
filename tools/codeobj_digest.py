"""Digest of the gfx950 code objects in a build's object directory.

  python tools/codeobj_digest.py socp.jl_amd/build/obj [more dirs ...]

For every *.o (sorted) the gfx950 code object is unbundled from the object's
.hip_fatbin section and the SHA-256 of
its .text, .rodata and .note sections printed, then from the metadata note one
line per kernel: VGPR, AGPR and SGPR counts and the private-segment (scratch)
size.  Two builds whose device code is the same print the same digest, so a
"same bits" change is checked with `diff` of two outputs.  (.dynstr is left
out: it holds a per-source hash symbol.)  It hashes and lists; nothing more."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SECTIONS = (".text", ".rodata", ".note")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def digest(obj, tmp):
    fb, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    try:
        tool("llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj)  # the host object's bundle of device code
    except subprocess.CalledProcessError:
        return ["  (host code only: no .hip_fatbin section)"]
    tool("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fb}", f"--output={co}")
    out = []
    for sec in SECTIONS:
        raw = os.path.join(tmp, "sec")
        tool("llvm-objcopy", "-O", "binary", f"--only-section={sec}", co, raw)
        with open(raw, "rb") as f:
            data = f.read()
        out.append(f"  {sec:8s} {len(data):9d} B  sha256 {hashlib.sha256(data).hexdigest()}")
    # the metadata note as llvm-readelf prints it: one "  - .key: value ..." block per kernel
    kernels = {}
    for block in re.split(r"\n  - (?=\.)", tool("llvm-readelf", "--notes", co)):
        kv = dict(re.findall(r"^\s*(\.\w+):\s+(\S+)\s*$", block, re.M))
        if ".name" in kv and all(f in kv for f in FIELDS if f != ".agpr_count"):
            kernels[kv[".name"]] = kv
    for name in sorted(kernels):
        kv = kernels[name]
        out.append(f"  {name}: vgpr {kv['.vgpr_count']} agpr {kv.get('.agpr_count', '0')} "
                   f"sgpr {kv['.sgpr_count']} scratch {kv['.private_segment_fixed_size']}")
    return out


def main(dirs):
    with tempfile.TemporaryDirectory() as tmp:
        for d in dirs:
            for fn in sorted(os.listdir(d)):
                if fn.endswith(".o"):
                    print(f"{os.path.basename(os.path.normpath(d))}/{fn}")
                    print("\n".join(digest(os.path.join(d, fn), tmp)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or ["socp.jl_amd/build/obj"])
