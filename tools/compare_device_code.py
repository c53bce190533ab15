#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libsfnative.so (a host-only refactor must leave it unchanged).

    tools/compare_device_code.py <before.so> <after.so>

The code objects are cut out of both fat binaries (as tests/test_kernel_resources.py does).  Reported: the two sets of kernel names,
every kernel's llvm-readelf --notes record (registers, spills, LDS, scratch, kernarg size) and every kernel's disassembly
(llvm-objdump -d, addresses stripped).  Exit status 0 when all three agree."""
import hashlib
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"


def code_objects(so):
    data = open(so, "rb").read()
    out = []
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data):
        b = m.start()
        num = struct.unpack_from("<Q", data, b + 24)[0]
        off = b + 32
        for _ in range(num):
            o, s, ts = struct.unpack_from("<QQQ", data, off)
            off += 24
            triple = data[off:off + ts].decode()
            off += ts
            if "gfx950" in triple and s > 0:
                out.append(data[b + o:b + o + s])
    return out


def kernels(so):
    """name -> (notes record as a sorted tuple, sha1 of the disassembly)"""
    res = {}
    for co in code_objects(so):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
            dis = subprocess.run([LLVM + "llvm-objdump", "-d", f.name], capture_output=True, text=True, check=True).stdout
        recs, cur = [], {}
        for ln in notes.split("\n"):
            m = re.match(r"\s+(?:- )?\.(\w+):\s+(.*)", ln)
            if not m:
                continue
            k, v = m.groups()
            if k == "agpr_count" and cur:
                recs.append(cur)
                cur = {}
            cur[k] = v.strip()
        recs.append(cur)
        lines = {}
        name = None
        for ln in dis.split("\n"):
            m = re.match(r"[0-9a-f]+ <(.+)>:$", ln)
            if m:
                name = m.group(1)
                lines[name] = []
            elif name and ln.strip():
                # instruction text without its address / encoding comment; branch targets are relative to the kernel's own symbol
                lines[name].append(re.sub(r"\s*//.*$", "", ln))
        code = {}
        for name, ls in lines.items():
            # a "..." that ENDS a symbol is objdump's mark for the zero fill behind the last kernel of a section: which kernel that is follows
            # the order of instantiation, and the fill is no instruction.  A "..." anywhere else counts
            while ls and ls[-1].strip() == "...":
                ls.pop()
            code[name] = hashlib.sha1("".join(ls).encode())
        for r in recs:
            if "name" in r and "vgpr_count" in r:
                n = r["name"]
                keep = tuple(sorted((k, v) for k, v in r.items() if k not in ("symbol",)))
                res[n] = (keep, code[n].hexdigest() if n in code else None)
    return res


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    notes_diff = [n for n in a if n in b and a[n][0] != b[n][0]]
    code_diff = [n for n in a if n in b and a[n][1] != b[n][1]]
    print("kernels: %d before, %d after; only before: %d, only after: %d" % (len(a), len(b), len(only_a), len(only_b)))
    print("notes records that differ: %d" % len(notes_diff))
    print("disassemblies that differ: %d" % len(code_diff))
    for n in only_a + only_b + notes_diff + code_diff:
        print("  ", n)
    return 1 if only_a or only_b or notes_diff or code_diff else 0


if __name__ == "__main__":
    sys.exit(main())
