#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of the same HIP objects, kernel symbol by kernel symbol (host only, no GPU):

    python codeobj_diff.py BEFORE_DIR AFTER_DIR igemm.o igemm_nt8s.o igemm_nt8h.o [--remarks BEFORE.log AFTER.log]

Per object: llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle for hipv4-amdgcn-amd-amdhsa--gfx950, then per kernel
  - the instruction bytes of its symbol (32-bit words that differ only as far as a symbol both objects have moved relative to the kernel
    -- pc-relative displacements of calls into shared device functions, layout addresses -- count as equal),
  - its 64-byte kernel descriptor without bytes 16..23 (the offset from the descriptor to the code: a layout address),
  - the resource line of its metadata note (VGPRs, AGPRs, SGPRs, static LDS, scratch bytes, spills).
It compares bytes and numbers only.  --remarks: the stderr of the two builds with -Rpass-analysis=kernel-resource-usage; for every kernel
that is not byte-identical the compiler's "Occupancy [waves/SIMD]" of both builds is printed too, and the kernel is marked WORSE when
scratch or spills went up, static LDS changed or the occupancy differs."""
import os
import re
import struct
import subprocess
import sys
import tempfile

import yaml

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
RES_KEYS = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
            ("scratch", ".private_segment_fixed_size"), ("vgpr_spill", ".vgpr_spill_count"), ("sgpr_spill", ".sgpr_spill_count")]


def device_elf(obj, tmp):
    fat = os.path.join(tmp, "fatbin")
    co = os.path.join(tmp, "gfx950.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}"], check=True)
    return co


def kernels(obj):
    """{kernel name: (instruction bytes, descriptor bytes without the code-entry offset, resource dict, {symbol: address - kernel address})}"""
    with tempfile.TemporaryDirectory() as tmp:
        co = device_elf(obj, tmp)
        data = open(co, "rb").read()
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    # ELF64 little endian: section headers, then the symbol table
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]     # name type flags addr off size link info align entsize
    symtab = next(s for s in secs if s[1] == 2)
    strtab = secs[symtab[6]]
    syms = {}
    for off in range(symtab[4], symtab[4] + symtab[5], 24):
        name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", data, off)
        end = data.index(b"\0", strtab[4] + name)
        syms[data[strtab[4] + name:end].decode()] = (info & 15, shndx, value, size)

    def body(sym):
        _, shndx, value, size = syms[sym]
        sec = secs[shndx]
        start = sec[4] + value - sec[3]
        return data[start:start + size]

    meta = yaml.safe_load(notes[notes.index("amdhsa.kernels:") - 0:].split("\n...")[0].replace("\t", " ")) if "amdhsa.kernels:" in notes else {}
    res = {k[".name"]: {short: k.get(key, 0) for short, key in RES_KEYS} for k in meta.get("amdhsa.kernels", [])}
    out = {}
    for name in res:
        kd = body(name + ".kd")
        assert len(kd) == 64 and syms[name][0] == 2, name
        out[name] = (body(name), kd[:16] + kd[24:], res[name], {s: v[2] - syms[name][2] for s, v in syms.items() if v[1] == syms[name][1]})
    return out


def same_code(a, b):
    """equal instruction bytes, or equal but for words whose difference is the distance some shared symbol moved relative to the kernel"""
    if a[0] == b[0]:
        return True
    if len(a[0]) != len(b[0]):
        return False
    moved = {(a[3][s] - b[3][s]) & 0xffffffff for s in set(a[3]) & set(b[3])}
    wa, wb = struct.unpack(f"<{len(a[0]) // 4}I", a[0]), struct.unpack(f"<{len(b[0]) // 4}I", b[0])
    return all(x == y or ((x - y) & 0xffffffff) in moved for x, y in zip(wa, wb))


def occupancies(log):
    """{kernel name: occupancy} from a -Rpass-analysis=kernel-resource-usage build log"""
    occ, name = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and name:
            occ[name] = int(m.group(1))
    return occ


def res_line(r):
    return " ".join(f"{k}={v}" for k, v in r.items())


def main(argv):
    remarks = None
    if "--remarks" in argv:
        i = argv.index("--remarks")
        remarks = (occupancies(argv[i + 1]), occupancies(argv[i + 2]))
        argv = argv[:i] + argv[i + 3:]
    before, after, objs = argv[0], argv[1], argv[2:]
    tot = same_tot = worse_tot = 0
    for o in objs:
        a, b = kernels(os.path.join(before, o)), kernels(os.path.join(after, o))
        missing, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        differ = [k for k in sorted(set(a) & set(b)) if not (same_code(a[k], b[k]) and a[k][1:3] == b[k][1:3])]
        same = len(set(a) & set(b)) - len(differ)
        print(f"{o}: {len(a)} kernels in the parent object, {len(b)} in the new one: {same} byte-identical (instructions, kernel descriptor apart "
              f"from its code-entry offset, resources), {len(differ)} not, {len(missing)} missing, {len(new)} new")
        for k in missing:
            print(f"  MISSING {k}")
        for k in new:
            print(f"  NEW {k}")
        for k in differ:
            ra, rb = a[k][2], b[k][2]
            bad = rb["scratch"] > ra["scratch"] or rb["vgpr_spill"] > ra["vgpr_spill"] or rb["sgpr_spill"] > ra["sgpr_spill"] or rb["lds"] != ra["lds"]
            oa = ob = ""
            if remarks:
                oa, ob = remarks[0].get(k), remarks[1].get(k)
                bad = bad or oa is None or oa != ob
                oa, ob = f" occupancy={oa}", f" occupancy={ob}"
            worse_tot += bad
            print(f"  {'WORSE' if bad else 'ok   '} {k}  (instruction bytes {len(a[k][0])} -> {len(b[k][0])})")
            print(f"      parent: {res_line(ra)}{oa}")
            print(f"      new:    {res_line(rb)}{ob}")
        tot += len(a)
        same_tot += same
    print(f"total: {tot} kernels in the parent objects, {same_tot} identical; of the others {worse_tot} break a resource condition "
          f"(scratch or spills up, static LDS changed, occupancy changed)")
    return 1 if worse_tot else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
