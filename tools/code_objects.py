#!/usr/bin/env python3
"""What the BUILT library holds, kernel by kernel (registers, LDS, scratch): the gfx950 code objects are cut out of the library's
.hip_fatbin section (clang offload bundles, one per translation unit) and their metadata notes read with llvm-readelf.
   python tools/code_objects.py [remo3d_amd/libremo3d_hip.so] [regex on the demangled name]
   python tools/code_objects.py --diff OLD.so NEW.so [regex]     kernel by kernel: is the device code of two builds the same?
tests/test_abi_cpu.py uses kernels() to assert that no kernel of ours touches scratch memory: round 4 found the patch kernel storing
48 bytes per lane there (an array of K sums chosen by a run-time index) - 70 MB per application at the headline size, with the
compiler's summary saying "vgpr-spill 0"."""
import hashlib
import itertools
import os
import re
import struct
import subprocess
import sys
import tempfile

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _section(path, name):
    out = subprocess.run([READELF, "-S", "-W", path], capture_output=True, text=True, check=True).stdout
    for line in out.splitlines():
        m = re.search(r"\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m and m.group(1) == name:
            return int(m.group(3), 16), int(m.group(4), 16)
    raise RuntimeError("no section %s in %s" % (name, path))


def code_objects(path):
    """[(target triple, bytes of the code object)] of every bundle in the library's .hip_fatbin section"""
    off, size = _section(path, ".hip_fatbin")
    with open(path, "rb") as f:
        f.seek(off)
        blob = f.read(size)
    found = []
    at = blob.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            o, s, t = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + t].decode()
            p += 24 + t
            if s and "amdgcn" in triple:
                found.append((triple, blob[at + o:at + o + s]))
        at = blob.find(MAGIC, at + len(MAGIC))
    return found


def kernels(path):
    """[{name, vgpr, sgpr, lds, scratch, triple, obj}] of every kernel of every gfx950 code object (number obj) in the library"""
    rows = []
    for obj, (triple, data) in enumerate(code_objects(path)):
        with tempfile.NamedTemporaryFile(suffix=".co") as tmp:
            tmp.write(data)
            tmp.flush()
            notes = subprocess.run([READELF, "--notes", tmp.name], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            def num(key):
                m = re.search(r"\.%s:\s+(\d+)" % key, block)
                return int(m.group(1)) if m else -1
            m = re.search(r"\.name:\s+(\S+)", block)
            if m:
                rows.append(dict(name=m.group(1), vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), lds=num("group_segment_fixed_size"),
                                 scratch=num("private_segment_fixed_size"), triple=triple, obj=obj))
    return rows


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(.*", "", d.replace("void ", "").replace("(anonymous namespace)::", "")) for d in out]


_PCREL = re.compile(r"(s_addc?_u32 s\d+, s\d+), (0x[0-9a-f]+|-?\d+)$")


def _no_addresses(ins):
    """The distance from the code to a constant table (the literal added to the program counter in the two instructions behind
    s_getpc_b64) is an address like any other: it follows the layout of the code object, not the kernel.  -> (instructions, count masked)"""
    out, masked = list(ins), 0
    for i, line in enumerate(ins):
        if line.startswith("s_getpc_b64"):
            for j in (i + 1, i + 2):
                if j < len(ins) and _PCREL.match(ins[j]):
                    out[j] = _PCREL.sub(r"\1, <pc-relative>", ins[j])
                    masked += 1
    return out, masked


def bodies(path):
    """{(code object number, mangled kernel name): (sha1 of its disassembly, instruction count, pc-relative literals masked)} over
    every gfx950 code object of the library.  The disassembly is llvm-objdump -d without addresses, encodings and symbol names (the comment behind
    every instruction) and without the pc-relative distances to constant data, so a kernel that only moved inside its code object
    hashes the same; branch targets are relative in the instruction text."""
    names = set(k["name"] for k in kernels(path))
    found = {}
    for obj, (_, data) in enumerate(code_objects(path)):
        with tempfile.NamedTemporaryFile(suffix=".co") as tmp:
            tmp.write(data)
            tmp.flush()
            text = subprocess.run([OBJDUMP, "-d", tmp.name], capture_output=True, text=True, check=True).stdout
        for part in re.split(r"^[0-9a-f]+ <", text, flags=re.M)[1:]:
            name, _, rest = part.partition(">:\n")
            if name in names:
                ins = [line.split("//")[0].strip() for line in rest.splitlines() if line.startswith("\t")]
                ins, masked = _no_addresses(ins)
                found[obj, name] = (hashlib.sha1("\n".join(ins).encode()).hexdigest(), len(ins), masked)
    return found


def _split(d):
    """demangled name -> (name without template arguments, [top-level template arguments])"""
    m = re.match(r"([^<]*)<(.*)>$", d)
    if not m:
        return d, []
    args, depth, cur = [], 0, ""
    for ch in m.group(2):
        depth += (ch in "<(") - (ch in ">)")
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return m.group(1), args + [cur.strip()]


def pairs(old, new):
    """[(old name or None, new name or None)] of two lists of demangled names: equal names, then - where a template has more arguments
    on one side - the names that are equal once the SAME argument positions are dropped from every kernel of that template."""
    out = [(d, d) for d in old if d in new]
    lo, ln = [d for d in old if d not in new], [d for d in new if d not in old]
    for base in sorted(set(_split(d)[0] for d in lo)):
        a = {d: _split(d)[1] for d in lo if _split(d)[0] == base}
        b = {d: _split(d)[1] for d in ln if _split(d)[0] == base}
        na, nb = set(map(len, a.values())), set(map(len, b.values()))
        if len(na) != 1 or len(nb) != 1 or na == nb:
            continue
        (long_, nl), (short, ns) = sorted([(a, na.pop()), (b, nb.pop())], key=lambda t: -t[1])
        def drop(pos):
            return [(dl, ds) for dl, al in long_.items() for ds, as_ in short.items() if [x for i, x in enumerate(al) if i not in pos] == as_]
        best = max((drop(pos) for pos in itertools.combinations(range(nl), nl - ns)), key=len)
        out += [(dl, ds) if long_ is a else (ds, dl) for dl, ds in best]
    seen_o, seen_n = set(o for o, _ in out), set(n for _, n in out)
    return out + [(d, None) for d in old if d not in seen_o] + [(None, d) for d in new if d not in seen_n]


def diff(old_lib, new_lib, filt="."):
    """prints one line per kernel that matches filt; returns how many of them differ or exist on one side only
    (a kernel that several translation units emit under one name - library templates - is 'name [2]', 'name [3]' .. in their order)"""
    side = []
    for lib in (old_lib, new_lib):
        ks, bs, seen = kernels(lib), bodies(lib), {}
        side.append({})
        for k, d in zip(ks, demangle([k["name"] for k in ks])):
            seen[d] = seen.get(d, 0) + 1
            side[-1][d if seen[d] == 1 else "%s [%d]" % (d, seen[d])] = (k, bs.get((k["obj"], k["name"]), ("-", -1, 0)))
    bad = total = 0
    for o, n in sorted(pairs(list(side[0]), list(side[1])), key=lambda t: t[1] or t[0]):
        if not re.search(filt, n or o):
            continue
        total += 1
        res = lambda k: "vgpr %3d sgpr %3d lds %6d scratch %4d" % (k["vgpr"], k["sgpr"], k["lds"], k["scratch"])
        if o is None or n is None:
            k, (_, cnt, _) = side[1][n] if o is None else side[0][o]
            verdict, what = ("only in NEW" if o is None else "only in OLD"), "%5d instructions  %s" % (cnt, res(k))
        else:
            (ko, (ho, co, _)), (kn, (hn, cn, mk)) = side[0][o], side[1][n]
            if ho == hn and res(ko) == res(kn):
                verdict, what = "identical", "%5d instructions  %s%s" % (cn, res(kn), "  (%d pc-relative offsets to data not compared)" % mk if mk else "")
            else:
                verdict, what = "DIFFERS", "%5d -> %5d instructions  %s -> %s" % (co, cn, res(ko), res(kn))
        bad += verdict != "identical"
        print("%-11s %-100s %s%s" % (verdict, (n or o)[:100], what, "   (was %s)" % o if o and n and o != n else ""))
    print("%d kernels compared, %d identical, %d not" % (total, total - bad, bad))
    return bad


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--diff":
        sys.exit(1 if diff(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else ".") else 0)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "remo3d_amd", "libremo3d_hip.so")
    filt = sys.argv[2] if len(sys.argv) > 2 else "."
    ks = kernels(lib)
    for k, d in zip(ks, demangle([k["name"] for k in ks])):
        if re.search(filt, d):
            print("%-90s vgpr %3d  sgpr %3d  lds %6d  scratch %4d" % (d[:90], k["vgpr"], k["sgpr"], k["lds"], k["scratch"]))
    print("%d kernels, %d with scratch" % (len(ks), sum(1 for k in ks if k["scratch"] > 0)))
