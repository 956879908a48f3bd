#!/usr/bin/env python3
"""Compare the machine code of the kernels of two builds of the device code, kernel by kernel.

  hipcc $(HIPFLAGS_CODE) --cuda-device-only -save-temps -c skirt9_amd/csrc/pmc_kernels.hip -o pmc_kernels.co     (in a directory per build)
  tools/kernel_code_diff.py A/pmc_kernels-hip-amdgcn-amd-amdhsa-gfx950.o B/pmc_kernels-hip-amdgcn-amd-amdhsa-gfx950.o [--skip trace,integrateRays]

The inputs are the relocatable objects that -save-temps leaves (before the link: what refers to another symbol is a zero field plus a
relocation, so the bytes of a kernel do not depend on where it or its neighbours end up).  Per function symbol the instruction bytes
and the relocations inside them (offset within the function, type, target symbol, addend) are compared.  Exit status 1 if any kernel that
both builds have differs, or if one build lacks a kernel of the other (names containing a --skip word are only listed)."""
import argparse
import hashlib
import struct
import sys


def functions(path):
    d = open(path, "rb").read()
    assert d[:6] == b"\x7fELF\x02\x01", "a little-endian ELF64 object is expected"
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]  # name type flags addr off size link info align entsize

    def cstr(table, at):
        base = sec[table][4]
        return d[base + at:d.index(b"\0", base + at)].decode()

    symtab = next(i for i, s in enumerate(sec) if s[1] == 2)
    syms = []
    for i in range(sec[symtab][5] // 24):
        name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", d, sec[symtab][4] + 24 * i)
        syms.append((cstr(sec[symtab][6], name), info & 15, shndx, value, size))
    relocs = {}  # per code section (template instantiations have one each)
    for s in sec:
        if s[1] == 4:  # SHT_RELA
            for j in range(s[5] // 24):
                off, info, addend = struct.unpack_from("<QQq", d, s[4] + 24 * j)
                relocs.setdefault(s[7], []).append((off, info & 0xFFFFFFFF, syms[info >> 32][0], addend))
    out = {}
    for name, kind, shndx, value, size in syms:
        if kind == 2 and 0 < shndx < shnum and sec[shndx][2] & 4 and size:  # a function in a section with SHF_EXECINSTR
            code = d[sec[shndx][4] + value:sec[shndx][4] + value + size]
            rel = sorted((o - value, t, n, a) for o, t, n, a in relocs.get(shndx, []) if value <= o < value + size)
            out[name] = (hashlib.sha256(code + repr(rel).encode()).hexdigest(), size)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--skip", default="", help="comma-separated words: kernels whose name contains one are not compared")
    args = ap.parse_args()
    skip = [w for w in args.skip.split(",") if w]
    A, B = functions(args.a), functions(args.b)
    same = differ = 0
    bad = []
    for name in sorted(set(A) | set(B)):
        if any(w in name for w in skip):
            print(f"skipped    {name}  {A.get(name, ('', '-'))[1]} -> {B.get(name, ('', '-'))[1]} bytes")
        elif name not in A or name not in B:
            bad.append(f"only in {'A' if name in A else 'B'}  {name}")
        elif A[name] != B[name]:
            differ += 1
            bad.append(f"DIFFERENT  {name}  {A[name][1]} -> {B[name][1]} bytes")
        else:
            same += 1
    print("\n".join(bad))
    print(f"{same} kernels identical, {differ} different, {len(bad) - differ} without a counterpart")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
