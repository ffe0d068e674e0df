#!/usr/bin/env python3
"""Digest of every gfx950 kernel in host objects: does a source change move any machine code?

usage: tools/kernel_digest.py [--by-content] OBJ... [--against OBJ...]

Each OBJ is a host object built by hipcc (build/*.o).  Its device code object is extracted with
`llvm-objcopy --dump-section .hip_fatbin` and `clang-offload-bundler --unbundle`; every kernel (a FUNC
symbol NAME with a kernel descriptor NAME.kd) prints as

    OBJ  SYMBOL  code bytes  sha1(code bytes)  the 64-byte descriptor in hex, its entry-offset field zeroed

(the entry offset is the distance from the descriptor to the code, which moves with everything else in the
unit).  With --against, the kernels of the first list are compared with those of the second as sets of
(symbol, size, digest, descriptor), whatever object each sits in; exit status 1 if they differ in any way.
--by-content pairs them by (size, digest, descriptor) alone, for a change that renames the symbols.
Bytes only: no instruction is inspected.
"""
import hashlib
import os
import shutil
import struct
import subprocess
import sys
import tempfile

ARCH = os.environ.get("BCMPC_ARCH", "gfx950")
STT_OBJECT, STT_FUNC = 1, 2


def tool(name):
    roots = [os.environ.get("ROCM_PATH", "/opt/rocm")]
    for r in roots:
        for sub in ("llvm/bin", "lib/llvm/bin", "bin"):
            p = os.path.join(r, sub, name)
            if os.access(p, os.X_OK):
                return p
    p = shutil.which(name)
    if not p:
        sys.exit(f"kernel_digest: {name} not found (set ROCM_PATH)")
    return p


def code_object(obj, tmp):
    """The gfx950 ELF inside a host object's .hip_fatbin section."""
    fat = os.path.join(tmp, "fat.bin")
    co = os.path.join(tmp, "dev.co")
    subprocess.run([tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")],
                   check=True)
    subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o",
                    f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}", f"--input={fat}", f"--output={co}"], check=True)
    with open(co, "rb") as f:
        return f.read()


def kernels(elf):
    """{symbol: (size, sha1 of the code bytes, masked descriptor hex)} of an AMDGPU ELF64 code object."""
    if elf[:6] != b"\x7fELF\x02\x01":
        raise ValueError("not a little-endian ELF64 code object")
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = []                                           # (type, addr, offset, size, link, entsize)
    for i in range(shnum):
        _, typ, _, addr, off, size, link, _, _, entsize = struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize)
        secs.append((typ, addr, off, size, link, entsize))
    syms = {}
    for typ, _, off, size, link, entsize in secs:
        if typ != 2:                                    # SHT_SYMTAB
            continue
        stroff = secs[link][2]
        for k in range(size // entsize):
            name, info, _, shndx, value, ssize = struct.unpack_from("<IBBHQQ", elf, off + k * entsize)
            if (info & 15) not in (STT_OBJECT, STT_FUNC) or shndx == 0 or shndx >= len(secs):
                continue
            end = elf.index(b"\0", stroff + name)
            _, saddr, soff, _, _, _ = secs[shndx]
            start = soff + value - saddr
            syms[elf[stroff + name:end].decode()] = (info & 15, elf[start:start + ssize])
    out = {}
    for name, (typ, code) in syms.items():
        kd = syms.get(name + ".kd")
        if typ != STT_FUNC or kd is None:
            continue
        desc = bytearray(kd[1])
        desc[16:24] = bytes(8)                          # kernel_code_entry_byte_offset
        out[name] = (len(code), hashlib.sha1(code).hexdigest(), desc.hex())
    return out


def digest(objs):
    rows = []
    for obj in objs:
        with tempfile.TemporaryDirectory() as tmp:
            for name, (size, sha, desc) in sorted(kernels(code_object(obj, tmp)).items()):
                rows.append((obj, name, size, sha, desc))
    return rows


def main(argv):
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0 if argv else 2
    by_content = "--by-content" in argv
    argv = [o for o in argv if o != "--by-content"]
    mine, theirs = (argv[:argv.index("--against")], argv[argv.index("--against") + 1:]) if "--against" in argv \
        else (argv, None)
    rows = digest(mine)
    for obj, name, size, sha, desc in rows:
        print(f"{obj}  {name}  {size}  {sha}  {desc}")
    for obj in mine:
        print(f"# {obj}: {sum(r[0] == obj for r in rows)} kernels")
    if theirs is None:
        return 0
    ref = digest(theirs)
    for obj in theirs:
        print(f"# against {obj}: {sum(r[0] == obj for r in ref)} kernels")
    a, b = sorted(r[1:] for r in rows), sorted(r[1:] for r in ref)
    if by_content:                                      # the symbols were renamed: pair the kernels by what they hold
        ca, cb = sorted(r[1:] for r in a), sorted(r[1:] for r in b)
        left = list(cb)
        for r in ca:
            if r in left:
                left.remove(r)
        same = len(cb) - len(left)
        print(f"# by content: {same} of {len(ca)} kernels have a kernel of the same size, code digest and descriptor "
              f"among the {len(cb)} of the second list")
        if same == len(ca) == len(cb):
            return 0
        for name, *r in a:
            if tuple(r) not in cb:
                print(f"# no match in the second list: {name}")
        for name, *r in b:
            if tuple(r) not in ca:
                print(f"# no match in the first list: {name}")
        print("# DIFFERENT")
        return 1
    if a == b:
        print(f"# identical: {len(a)} kernels, every symbol, size, code digest and descriptor")
        return 0
    da, db = {r[0]: r for r in a}, {r[0]: r for r in b}
    for name in sorted(set(da) | set(db)):
        if name not in db:
            print(f"# only in the first list: {name}")
        elif name not in da:
            print(f"# only in the second list: {name}")
        elif da[name] != db[name]:
            what = [w for w, i in (("size", 1), ("code", 2), ("descriptor", 3)) if da[name][i] != db[name][i]]
            print(f"# differs ({', '.join(what)}): {name}")
    if len(a) != len(set(r[0] for r in a)) or len(b) != len(set(r[0] for r in b)):
        print("# a kernel sits in more than one object of a list")
    print("# DIFFERENT")
    return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
