"""Measurement aid: which kernels of two builds differ, e.g.
    python3 tools/kernel_isa_diff.py parent/libsbmbp_hip.so sbm-bp_amd/csrc/libsbmbp_hip.so
OLD and NEW are two built libraries or two device-only objects (hipcc --cuda-device-only -c). Per kernel symbol of every
gfx code object inside: SAME when the disassembly (addresses and encodings stripped) is identical, else the two resource
tuples from the AMDGPU metadata notes. Symbols on one side only are listed, and only they make the exit status nonzero.
The comparison is of whole texts by digest: the tool looks at no particular instruction."""
import hashlib
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
EM_AMDGPU = 224
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
HEAD = ("vgpr", "agpr", "sgpr", "lds", "scratch", "vspill", "sspill")


def device_elfs(path):
    """the gfx code objects of a fat binary (the host ELF in front of them is skipped by its machine type), or the file
    itself where it is a device-only object"""
    data = open(path, "rb").read()
    out = []
    for m in re.finditer(b"\x7fELF\x02\x01\x01", data):
        h = data[m.start():m.start() + 64]
        if len(h) < 64 or struct.unpack_from("<H", h, 18)[0] != EM_AMDGPU:
            continue
        shoff, = struct.unpack_from("<Q", h, 40)
        shentsize, shnum = struct.unpack_from("<HH", h, 58)
        out.append(data[m.start():m.start() + shoff + shentsize * shnum])
    return out


def kernels(path):
    """{"<code object index>:<symbol>": (resource tuple, digest of the disassembly)}"""
    out = {}
    for n, elf in enumerate(device_elfs(path)):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(elf)
            f.flush()
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
            asm = subprocess.run([LLVM + "llvm-objdump", "-d", f.name], capture_output=True, text=True, check=True).stdout
        res = {}
        for blk in notes.split("- .agpr_count:")[1:]:
            blk = ".agpr_count:" + blk
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            res[name] = tuple(int(g.group(1)) if g else 0 for g in (re.search(r"\.%s:\s+(\d+)" % k, blk) for k in FIELDS))
        text = {}
        cur = None
        for line in asm.splitlines():
            m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
            if m:
                cur = text.setdefault(m.group(1), hashlib.sha256())
            elif cur is not None and line.strip():
                cur.update(line.split("//")[0].strip().encode() + b"\n")
        for name, r in res.items():
            if name not in text:
                sys.exit("%s: kernel %s is in the metadata notes of code object %d but not in its disassembly" % (path, name, n))
            out["%d:%s" % (n, name)] = (r, text[name].hexdigest())
    return out


def demangle(names):
    syms = [x.split(":", 1)[1] for x in names]
    got = subprocess.run(["c++filt"] + syms,capture_output=True, text=True).stdout.splitlines() if syms else []
    # template arguments stay, the parameter list goes
    return {x: x.split(":")[0] + ":" + re.sub(r"^void ", "", d).split("(")[0] for x, d in zip(names, got)}


def main(old, new):
    a, b = kernels(old), kernels(new)
    both = sorted(set(a) & set(b))
    pretty = demangle(sorted(set(a) | set(b)))
    differ = [k for k in both if a[k][1] != b[k][1]]
    for k in both:
        if k not in differ:
            print("SAME  %s" % pretty[k])
    if differ:
        print("\nDIFFER (%s): old -> new" % " ".join(HEAD))
        for k in differ:
            print("DIFF  %-70s %s -> %s" % (pretty[k], " ".join(map(str, a[k][0])), " ".join(map(str, b[k][0]))))
    for side, only in (("OLD", sorted(set(a) - set(b))), ("NEW", sorted(set(b) - set(a)))):
        for k in only:
            print("ONLY IN %s  %s" % (side, pretty[k]))
    print("\n%d kernels: %d same, %d differ, %d only in old, %d only in new" % (len(set(a) | set(b)), len(both) - len(differ), len(differ), len(set(a) - set(b)), len(set(b) - set(a))))
    return 1 if set(a) != set(b) else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
