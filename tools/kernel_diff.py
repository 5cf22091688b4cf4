#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the library kernel by kernel.

    tools/kernel_diff.py BUILD_DIR_A BUILD_DIR_B [--resources PATTERN]

Each directory holds the object files of one build (min_llm_inference_amd/build).  Every object's device code object is
unbundled and disassembled; per kernel symbol the instruction text (addresses and encodings dropped) is hashed.  Prints
the kernels present in both builds whose code differs and the kernels only one build has; exits 1 when a kernel present
in both differs.  With --resources, also prints VGPR / AGPR / scratch / LDS of B's kernels whose name contains PATTERN,
from the code object's metadata notes.  Needs no GPU."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(obj, tmp):
    fat = os.path.join(tmp, "fat.bin")
    out = os.path.join(tmp, os.path.basename(obj) + ".co")
    r = subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.devnull], capture_output=True)
    if r.returncode != 0 or not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}",
                        f"--output={out}"], capture_output=True, text=True)
    os.remove(fat)
    return out if r.returncode == 0 and os.path.getsize(out) > 0 else None


def kernels(build_dir):
    """{symbol: sha1 of its instruction text}, {symbol: metadata dict}"""
    code, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(os.listdir(build_dir)):
            if not name.endswith(".o"):
                continue
            co = code_object(os.path.join(build_dir, name), tmp)
            if co is None:
                continue
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                 capture_output=True, text=True, check=True).stdout
            sym, lines = None, []
            for line in dis.splitlines() + ["<end>:"]:
                m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line.strip())
                if m or line == "<end>:":
                    if sym is not None and not sym.startswith("L"):
                        code[sym] = hashlib.sha1("\n".join(lines).encode()).hexdigest()
                    sym, lines = (m.group(1) if m else None), []
                elif sym is not None:
                    text = re.sub(r"//.*$", "", line).strip()
                    if text and text != "..." and text not in ("s_nop 0", "s_code_end"):   # padding between kernels
                        lines.append(text)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count:")[1:]:
                block = ".agpr_count:" + block
                get = lambda key: (re.search(rf"\.{key}:\s*(\S+)", block) or [None, "?"])[1]
                meta[get("name")] = {k: get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size",
                                                           "group_segment_fixed_size")}
    return code, meta


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    a, _ = kernels(argv[1])
    b, meta = kernels(argv[2])
    both = sorted(set(a) & set(b))
    differ = [k for k in both if a[k] != b[k]]
    print(f"{len(a)} kernels in A, {len(b)} in B, {len(both)} in both, {len(differ)} of them differ")
    for k in differ:
        print("  differs:", k)
    for k in sorted(set(a) - set(b)):
        print("  only in A:", k)
    for k in sorted(set(b) - set(a)):
        print("  only in B:", k)
    if "--resources" in argv:
        pat = argv[argv.index("--resources") + 1]
        for k in sorted(meta):
            if pat in k:
                print("  ", k, meta[k])
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
