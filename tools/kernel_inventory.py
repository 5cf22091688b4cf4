#!/usr/bin/env python3
"""The device kernels of a build of the library, by demangled name.

    tools/kernel_inventory.py BUILD_DIR

BUILD_DIR holds the object files of one build (min_llm_inference_amd/build).  Every object's gfx950 code object is unbundled
(tools/kernel_diff.py), its symbol table read, and the kernel symbols kept: a kernel is a function with a kernel descriptor,
the object symbol NAME.kd next to it.  The names are demangled (llvm-cxxfilt of the ROCm LLVM; binutils' c++filt where that
installation ships none), normalised (normalise() below: the key under which tests/kernel_coverage.json records which test files
launch the kernel) and printed one per line, sorted.  Needs no GPU."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_diff import LLVM, code_object  # noqa: E402


def demangler():
    for tool in (os.path.join(LLVM, "llvm-cxxfilt"), shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if tool and os.path.exists(tool):
            return tool
    raise RuntimeError(f"no demangler: neither {LLVM}/llvm-cxxfilt nor c++filt")


def demangle(names):
    """the demangled form of every name, in order (names that are not mangled come back unchanged)"""
    names = list(names)
    if not names:
        return []
    out = subprocess.run([demangler()], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    lines = out.split("\n")[:len(names)]
    assert len(lines) == len(names)
    return lines


def normalise(name):
    """One key per kernel, whichever tool named it: the symbol table's NAME.kd or NAME (demangled by either demangler, which
    differ in the spacing of `> >` and in a `[clone .kd]` note) and the profiler's Kernel_Name column (demangled already, with
    or without the .kd suffix; a mangled one is demangled here).  Template arguments and the parameter list stay: they are what
    tells two instantiations apart."""
    name = name.strip().strip('"')
    if name.endswith(".kd"):
        name = name[:-3]
    if name.startswith("_Z"):
        name = demangle([name])[0]
    name = re.sub(r"\s*\[clone \.kd\]\s*$", "", name)
    if name.endswith(".kd"):
        name = name[:-3]
    name = re.sub(r"\s+", " ", name).strip()
    name = re.sub(r"\s*([<>,()*&])\s*", r"\1", name)          # `> >` and `>>`, `, ` and `,`, `const *` and `const*`
    return name.replace(",", ", ")


def kernel_symbols(build_dir):
    """the mangled kernel symbols of every object file of the build, sorted"""
    found = set()
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(os.listdir(build_dir)):
            if not obj.endswith(".o"):
                continue
            co = code_object(os.path.join(build_dir, obj), tmp)
            if co is None:
                continue
            table = subprocess.run([f"{LLVM}/llvm-readelf", "--symbols", "--wide", co], capture_output=True, text=True,
                                   check=True).stdout
            symbols = {}
            for line in table.splitlines():
                f = line.split()
                if len(f) == 8 and f[0].endswith(":") and f[0][:-1].isdigit():
                    symbols[f[7]] = f[3]
            found |= {s[:-3] for s, kind in symbols.items() if s.endswith(".kd") and kind == "OBJECT" and symbols.get(s[:-3]) == "FUNC"}
    return sorted(found)


def inventory(build_dir):
    """the normalised demangled kernel names of the build, sorted"""
    return sorted({normalise(n) for n in demangle(kernel_symbols(build_dir))})


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    print("\n".join(inventory(sys.argv[1])))
