"""Do two builds hold the same gfx950 kernels, instruction for instruction?  CPU only.

usage: python bench/isa_diff.py OLD NEW
       OLD, NEW: a built _kernels shared object, or a directory of .o files

Every gfx950 code object of every clang offload bundle is disassembled with ROCm's llvm-objdump
and every function is keyed by its mangled name, whichever code object it sits in (a kernel that
moved to another translation unit keeps its key).  Compared are the instruction streams, after
comments and directives are dropped and local labels .LBB<k>_<n> are renumbered in order of
appearance.  Prints the names only in OLD, only in NEW and the names whose streams differ; the
exit status is non-zero on any difference.
"""
import collections
import glob
import os
import re
import struct
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"
LABEL = re.compile(r"\.LBB\d+_\d+")


def code_objects(path):
    """gfx950 ELF code objects of every (uncompressed) clang offload bundle in the file."""
    d = open(path, "rb").read()
    i = d.find(BUNDLE)
    while i >= 0:
        n = struct.unpack_from("<Q", d, i + 24)[0]
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", d, p)
            p += 24
            if b"gfx950" in d[p:p + tl]:
                yield d[i + off:i + off + size]
            p += tl
        i = d.find(BUNDLE, i + len(BUNDLE))


def normalise(body):
    ids = {}
    out = []
    for line in body:
        line = re.split(r"//|;", line)[0].strip()
        if not line or (line.startswith(".") and not LABEL.match(line)):
            continue
        out.append(LABEL.sub(lambda m: ids.setdefault(m.group(0), f".L{len(ids)}"), line))
    return tuple(out)


def kernels(path):
    """mangled name -> sorted instruction streams (one per code object that defines the name)"""
    files = sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]
    funcs = collections.defaultdict(list)
    with tempfile.TemporaryDirectory() as td:
        for f in files:
            for co in code_objects(f):
                elf = os.path.join(td, "co.elf")
                open(elf, "wb").write(co)
                txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", elf], capture_output=True, text=True,
                                     check=True).stdout
                name, body = None, []
                for line in txt.splitlines() + ["0 <>:"]:
                    m = re.match(r"^[0-9a-f]+ <(\S*)>:$", line)
                    if m:
                        if name:
                            funcs[name].append(normalise(body))
                        name, body = m.group(1), []
                    elif name and line.startswith("\t"):
                        body.append(line)
    assert funcs, "no gfx950 code object found in " + path
    return {k: sorted(v) for k, v in funcs.items()}


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    for title, names in (("only in OLD", only_old), ("only in NEW", only_new), ("streams differ", differ)):
        print(f"{title}: {len(names)}")
        for k in names:
            print("  " + k)
    for k in differ[:1]:   # where the first differing kernel diverges
        a, b = old[k][0], new[k][0]
        i = next((j for j, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f"first difference of {k}: instruction {i} of {len(a)} / {len(b)}: {a[i:i + 1]} -> {b[i:i + 1]}")
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {len(set(old) & set(new)) - len(differ)} identical")
    return 1 if only_old or only_new or differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
