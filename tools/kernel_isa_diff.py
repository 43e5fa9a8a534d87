"""Compare the gfx950 device code of two builds of the library, kernel by kernel, without a GPU.

    python tools/kernel_isa_diff.py OLD.so NEW.so

Each library's gfx950 code objects are extracted (llvm-objdump --offloading, as tests/test_cabi.py does) and disassembled; the
text is split at the function symbols, names are demangled, addresses (the pc-relative ones of constant tables included) and
encoding bytes are dropped, and what is left -- mnemonic and operands, line by line -- is compared per kernel, together with the
kernel's .vgpr_count, .sgpr_count, .group_segment_fixed_size and .private_segment_fixed_size from the code object's notes.
Prints the kernels that differ, the kernels present on one side only and a final count line; exit status 1 if a kernel present on
both sides differs.  The two always-false template parameters that sepup_pipe_kernel used to carry in front of VCOL are dropped
from old names before the two sides are matched.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("PF_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
META = (".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_count", ".vgpr_count")


def _run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, capture_output=True, text=True).stdout


def canonical(name):
    """sepup_pipe_kernel<BN, W, D, W_BY_PROD, DEFER, false, false, VCOL> -> <BN, W, D, W_BY_PROD, DEFER, VCOL>."""
    return re.sub(r"(sepup_pipe_kernel<\d+, \d+, \d+, \w+, \w+), false, false, (\w+>)", r"\1, \2", name)


def strip_pc_relative(lines):
    """s_getpc_b64 s[N:N+1]; s_add_u32 sN, sN, LITERAL; s_addc_u32 sN+1, sN+1, LITERAL is the address of a constant table relative to
    the instruction: a linked address like the ones dropped with the encodings (it moves with the size of the symbol tables)."""
    lo = hi = None
    for k, line in enumerate(lines):
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]$", line)
        if m:
            lo, hi = "s" + m.group(1), "s" + m.group(2)
        elif lo and re.match(r"s_add_u32 %s, %s, " % (lo, lo), line):
            lines[k], lo = "s_add_u32 %s, %s, <pc-relative>" % (lo, lo), None
        elif hi and re.match(r"s_addc_u32 %s, %s, " % (hi, hi), line):
            lines[k], hi = "s_addc_u32 %s, %s, <pc-relative>" % (hi, hi), None


def kernels_of(lib):
    """{demangled name: (instruction lines, {metadata key: value} or None for a function that is no kernel)}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "lib.so")                 # --offloading extracts next to its input
        shutil.copy(lib, copy)
        _run("llvm-objdump", "--offloading", copy)
        objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if "gfx950" in f)
        if not objs:
            sys.exit("%s: no gfx950 code object" % lib)
        for co in objs:
            meta, rec = {}, None
            for line in _run("llvm-readelf", "--notes", co).splitlines():
                m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s+(\S+)", line)
                if not m:
                    continue
                key, val = m.groups()
                if key == ".group_segment_fixed_size":     # first of a kernel's keys behind its argument list
                    rec = {}
                if rec is not None and key in META:
                    rec[key] = int(val)
                if rec is not None and key == ".symbol":
                    meta[val[:-3] if val.endswith(".kd") else val] = rec
                if key == ".vgpr_count":                   # last of them
                    rec = None
            body, sym = {}, None
            for line in _run("llvm-objdump", "-d", co).splitlines():
                m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
                if m:
                    sym = m.group(1)
                    body[sym] = []
                elif sym is not None and line.strip():
                    body[sym].append(" ".join(line.split("//")[0].split()))
            for lines in body.values():
                strip_pc_relative(lines)
            # the same listing with demangled labels (--demangle; the notes name kernels by their mangled symbols), in the same order
            names = re.findall(r"^[0-9a-f]+ <(.+)>:$", _run("llvm-objdump", "-d", "--demangle", co), flags=re.M)
            assert len(names) == len(body)
            for sym, name in zip(body, names):
                name = canonical(name)
                assert name not in out, "duplicate symbol " + name
                out[name] = (body[sym], meta.get(sym))
    return out


def main(old_lib, new_lib):
    old, new = kernels_of(old_lib), kernels_of(new_lib)
    print("old: %s (%d functions, %d kernels)\nnew: %s (%d functions, %d kernels)"
          % (old_lib, len(old), sum(m is not None for _, m in old.values()), new_lib, len(new), sum(m is not None for _, m in new.values())))
    differ = 0
    for name in sorted(set(old) & set(new)):
        (oi, om), (ni, nm) = old[name], new[name]
        why = []
        if oi != ni:
            first = next((k for k, (x, y) in enumerate(zip(oi, ni)) if x != y), min(len(oi), len(ni)))
            why.append("instructions: %d -> %d lines, first difference at line %d: %r -> %r"
                       % (len(oi), len(ni), first, oi[first] if first < len(oi) else None, ni[first] if first < len(ni) else None))
        if om != nm:
            why.append("metadata: %s -> %s" % (om, nm))
        if why:
            differ += 1
            print("DIFFERS  %s\n         %s" % (name, "\n         ".join(why)))
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    for name in only_old:
        print("OLD ONLY %s" % name)
    for name in only_new:
        print("NEW ONLY %s" % name)
    print("%d compared, %d differ, %d in old only, %d in new only" % (len(set(old) & set(new)), differ, len(only_old), len(only_new)))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
