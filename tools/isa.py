"""Disassembly of the gfx950 code object inside a built libmatfact_hip.so (llvm-objdump from /opt/rocm/lib/llvm/bin).

Used by tests/test_isa.py (the hand-written ISA invariants of the kernels, checked on the CPU) and as a command:
    python tools/isa.py [lib.so]                 per-kernel instruction census
    python tools/isa.py [lib.so] <symbol part>   the instructions of every kernel whose demangled name contains the part
    python tools/isa.py --compare PARENT.so NEW.so [name part]
                                                 per kernel `same`, `ok` or `MISS` (compare() below) with what differs:
                                                 the table a refactor of the kernels is judged by
Nothing here is on the product path."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "recommender-system_amd", "csrc", "libmatfact_hip.so")
LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def _tool(name):
    p = os.path.join(LLVM_BIN, name)
    return p if os.path.exists(p) else shutil.which(name)


def have_tools():
    return _tool("llvm-objdump") is not None and _tool("llvm-readelf") is not None and shutil.which("c++filt") is not None


def _extract(lib, tmp):
    """path of the gfx950 code object of `lib`, extracted into the directory `tmp`"""
    local = os.path.join(tmp, "lib.so")
    shutil.copy(lib, local)   # --offloading writes the extracted bundles beside its input
    subprocess.check_call([_tool("llvm-objdump"), "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
    objs = [f for f in os.listdir(tmp) if "gfx950" in f]
    if not objs:
        raise RuntimeError("no gfx950 code object in " + lib)
    return os.path.join(tmp, objs[0])


def _demangle(names):
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()


def metadata(lib=DEFAULT_LIB):
    """{demangled kernel name: {'.vgpr_count': 34, '.private_segment_fixed_size': 0, ...}} from the code object's notes"""
    with tempfile.TemporaryDirectory() as tmp:
        text = subprocess.check_output([_tool("llvm-readelf"), "--notes", _extract(lib, tmp)], text=True)
    kernels, cur = [], None
    for line in text.splitlines():
        m = re.match(r"^\s+(-\s)?(\.[a-z_]+):\s+(\S+)\s*$", line)
        if line.startswith("  - .") and m:
            cur = {}
            kernels.append(cur)
        if m and cur is not None and len(line) - len(line.lstrip()) <= 4:
            v = m.group(3)
            cur[m.group(2)] = int(v) if re.fullmatch(r"-?\d+", v) else v
    dem = _demangle([k.get(".name", "?") for k in kernels])
    return dict(zip(dem, kernels))


def disassemble(lib=DEFAULT_LIB):
    """{demangled kernel name: [instruction text, ...]} of the gfx950 code object bundled in `lib`."""
    with tempfile.TemporaryDirectory() as tmp:
        text = subprocess.check_output([_tool("llvm-objdump"), "-d", "--mcpu=gfx950", _extract(lib, tmp)], text=True)
    names, bodies, cur = [], [], None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            names.append(m.group(1))
            cur = []
            bodies.append(cur)
            continue
        if cur is None:
            continue
        ins = line.split("//")[0].strip()
        if ins:
            cur.append(ins)
    return dict(zip(_demangle(names), bodies))


_REG = re.compile(r"\b([vsa])(?:(\d+)|\[(\d+):(\d+)\])")


def regs(operand_text, kind="v"):
    """set of register numbers of one kind named in an operand string: 'v[6:9], v12' -> {6, 7, 8, 9, 12}"""
    out = set()
    for k, one, lo, hi in _REG.findall(operand_text):
        if k != kind:
            continue
        if one:
            out.add(int(one))
        else:
            out.update(range(int(lo), int(hi) + 1))
    return out


def split(ins):
    """('v_add_f64', 'v[0:1], v[2:3], v[4:5]')"""
    parts = ins.split(None, 1)
    return parts[0], (parts[1] if len(parts) > 1 else "")


def census(body):
    c = {}
    for ins in body:
        op = split(ins)[0]
        c[op] = c.get(op, 0) + 1
    return c


# scalar ALU, compare and branch, and the s_nop padding hipcc places itself: free to move in a refactor
_SCALAR_FREE = re.compile(r"s_(nop|branch|cbranch|cmp|cmpk|cselect|cmov|mov|movk|add|addc|addk|sub|subb|mul|mulk|and|andn\d|or|orn\d|xor|"
                          r"xnor|nand|nor|not|lshl|lshr|ashr|bfe|bfm|min|max|abs|sext|ff[01]|flbit|bcnt|brev|bitset|bitcmp|wqm|"
                          r"quadmask|pack|getpc|setpc|swappc)(_|$)")
_FIXED_HEAD = re.compile(r"(global_|flat_|buffer_|scratch_|ds_|s_load|s_buffer_load|s_waitcnt|s_barrier)")
_META = (".vgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def _int_or_move(op):
    return op.startswith("v_") and not op.startswith("v_mfma") and not re.search(r"_(f16|bf16|f32|f64)", op)


def compare(pbody, pmeta, nbody, nmeta):
    """('same' | 'ok' | 'MISS', [what differs]) of one kernel, parent against new.
    same: equal instruction list and metadata.
    ok:   VGPR, spill, scratch and LDS figures equal, SGPR count no higher; from the first v_mfma to the end (reported as
          `stream` up to the last v_mfma and `tail` behind it) every opcode count equal but for scalar ALU / compare /
          branch and s_nop; before it (`head`: once per workgroup; the whole body of a kernel without matrix instructions)
          memory, LDS, wait and barrier counts equal, only integer arithmetic and move opcodes differ otherwise, and at
          most 4 vector instructions more than the parent."""
    if pbody == nbody and pmeta == nmeta:
        return "same", []
    notes, ok = [], True
    for k in _META + (".sgpr_count",):
        a, b = pmeta.get(k), nmeta.get(k)
        if a != b:
            notes.append("%s %s -> %s" % (k, a, b))
            ok &= k == ".sgpr_count" and b <= a
    def spans(body):   # before the first matrix instruction, up to the last one, behind it (a tile's epilogue and the kernel's end)
        mf = [i for i, x in enumerate(body) if x.startswith("v_mfma")]
        return (body, [], []) if not mf else (body[:mf[0]], body[mf[0]:mf[-1] + 1], body[mf[-1] + 1:])
    for span, pb, nb in zip(("head", "stream", "tail"), spans(pbody), spans(nbody)):
        pc, nc = census(pb), census(nb)
        for op in sorted(set(pc) | set(nc)):
            a, b = pc.get(op, 0), nc.get(op, 0)
            if a == b or not op[0].isalpha():   # "...": padding the disassembler skips
                continue
            notes.append("%s %s %d -> %d" % (span, op, a, b))
            if _SCALAR_FREE.match(op):
                continue
            ok &= span == "head" and not _FIXED_HEAD.match(op) and _int_or_move(op)
        if span == "head":
            pv, nv = (sum(n for op, n in c.items() if op.startswith("v_")) for c in (pc, nc))
            if nv > pv + 4:
                notes.append("head vector instructions %d -> %d" % (pv, nv))
                ok = False
    if not notes:
        notes.append("equal opcode counts and metadata; operands or order differ")
    return ("ok" if ok else "MISS"), notes


def _compare_main(parent, new, part):
    pk, nk, pm, nm = disassemble(parent), disassemble(new), metadata(parent), metadata(new)
    print("kernels: %d in %s, %d in %s" % (len(pk), parent, len(nk), new))
    only = sorted(set(pk) ^ set(nk))
    for n in only:
        print("ONLY IN %s: %s" % ("PARENT" if n in pk else "NEW", n))
    tally = {}
    for name in sorted(set(pk) & set(nk)):
        if part and part not in name:
            continue
        verdict, notes = compare(pk[name], pm.get(name, {}), nk[name], nm.get(name, {}))
        tally[verdict] = tally.get(verdict, 0) + 1
        if verdict != "same" or part:
            print("%-5s %s" % (verdict, name))
            for x in notes:
                print("        " + x)
    print("total: " + ", ".join("%d %s" % (tally[v], v) for v in ("same", "ok", "MISS") if v in tally) +
          (", %d on one side only" % len(only) if only else ""))
    return 1 if tally.get("MISS") or only else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--compare":
        sys.exit(_compare_main(args[1], args[2], args[3] if len(args) > 3 else None))
    lib = DEFAULT_LIB
    if args and args[0].endswith(".so"):
        lib = args.pop(0)
    kernels = disassemble(lib)
    if args:
        for name, body in kernels.items():
            if args[0] in name:
                print("//", name, len(body), "instructions")
                print("\n".join(body))
    else:
        for name, body in kernels.items():
            if "rocprim" in name:
                continue
            c = census(body)
            pick = {k: v for k, v in c.items() if k.startswith(("v_fma", "v_fmac", "v_mfma", "scratch_", "global_load_lds", "ds_read_b128", "buffer_"))}
            print("%-70s %6d  %s" % (name[:70], len(body), pick))
