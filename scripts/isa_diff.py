"""Do two builds hold the same device code?  python scripts/isa_diff.py OBJDIR_A OBJDIR_B [name filter]

For every .o of the two object directories: the gfx950 code object is unbundled, disassembled (llvm-objdump -d --no-show-raw-insn
--no-leading-addr) and split per symbol; a kernel is the same if its instruction text and its metadata tuple (VGPRs, AGPRs, SGPRs, VGPR
and SGPR spills, private segment, group segment, kernel-argument segment, and where it lies in its code object: offset and size, since
the same instructions at another address meet the instruction cache differently) are.  One line per kernel that differs or exists on one
side only, then a summary line; exit status 1 if anything differs.  The text is compared wholesale: no instruction is looked for."""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size", "text_offset", "text_size")


def _run(*cmd):
    """Output of a tool that has to succeed: a tool failing alike on both sides would make them compare equal."""
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("isa_diff: %s failed (%d)\n%s" % (" ".join(cmd), r.returncode, r.stderr))
    return r.stdout


def code_object(obj, tmpdir):
    """Path of the gfx950 code object embedded in a host object (None: the object has no .hip_fatbin section)."""
    if not re.search(r"\s\.hip_fatbin\s", _run(os.path.join(LLVM, "llvm-readelf"), "-SW", obj)):
        return None
    base = os.path.join(tmpdir, os.path.basename(obj))
    fb, co = base + ".fatbin", base + ".co"
    _run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, obj)
    _run(os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + fb, "--output=" + co, "--unbundle")
    if not (os.path.exists(co) and os.path.getsize(co)):
        sys.exit("isa_diff: no %s code object in %s" % (TARGET, obj))
    return co


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"^void ", "", d).split("(")[0] for n, d in zip(names, out)}


def metadata(co):
    """{mangled kernel name: {metadata key: value}} from the code object's notes."""
    kernels, where = {}, {}
    for line in _run(os.path.join(LLVM, "llvm-readelf"), "-sW", co).split("\n"):
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            where[f[7]] = (str(int(f[1], 16)), f[2])
    for blk in _run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        get = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, "?"])[1]
        kernels[get("name")] = {k: get(k) for k in META[:-2]}
        kernels[get("name")]["text_offset"], kernels[get("name")]["text_size"] = where.get(get("name"), ("?", "?"))
    return kernels


def disassembly(co):
    """{symbol: [instruction text, ...]} -- addresses, encodings and the address comments left out."""
    syms, cur = {}, None
    for line in _run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).split("\n"):
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return syms


def kernels_of(objdir, tmpdir):
    """{(object file, mangled name): (metadata dict, instructions)} of every kernel of every object in objdir."""
    objs = sorted(o for o in os.listdir(objdir) if o.endswith(".o"))

    def one(o):
        co = code_object(os.path.join(objdir, o), tmpdir)
        if not co:
            return o, {}
        dis, meta = disassembly(co), metadata(co)
        if not meta or not all(dis.get(name) for name in meta):
            sys.exit("isa_diff: %s has device code but %s" % (o, "a kernel without instructions" if meta else "no kernels"))
        return o, {name: (m, dis[name]) for name, m in meta.items()}

    with ThreadPoolExecutor(min(8, max(1, len(objs)))) as pool:
        return {(o, name): v for o, ks in pool.map(one, objs) for name, v in ks.items()}


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    flt = argv[3] if len(argv) > 3 else ""
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        A, B = kernels_of(argv[1], ta), kernels_of(argv[2], tb)
    pretty = demangle(sorted({n for _, n in list(A) + list(B)}))
    keys = [k for k in sorted(set(A) | set(B)) if flt in pretty[k[1]]]
    tup = lambda meta: " ".join("%s %s" % (k.replace("_count", "").replace("_fixed_size", "").replace("_segment", ""), meta[k]) for k in META)
    differ = missing = extra = 0
    for k in keys:
        where = "%-14s %s" % (k[0], pretty[k[1]])
        if k not in B:
            missing += 1
            print("only in A  %s" % where)
        elif k not in A:
            extra += 1
            print("only in B  %s" % where)
        elif A[k] != B[k]:
            differ += 1
            (ma, ia), (mb, ib) = A[k], B[k]
            print("differs    %s\n           A: %6d instructions  %s\n           B: %6d instructions  %s" % (where, len(ia), tup(ma), len(ib), tup(mb)))
    objs = len({o for o, _ in keys})
    insts = sum(len(A[k][1]) for k in keys if k in A)
    print("isa_diff: %d kernels in %d objects compared (%d instructions on side A): %d differing, %d missing, %d extra"
          % (len(keys), objs, insts, differ, missing, extra))
    return 1 if differ or missing or extra or not keys else 0      # (nothing compared is no pass)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
