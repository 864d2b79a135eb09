#!/usr/bin/env python3
"""dev: is the device code of two builds of libmythos_hip.so the same?  The gate of a refactor that moves device text.

usage: isa_diff.py [--table] [--alias REGEX=REPL] parent.so branch.so      exit code 0: identical, 1: something differs (listed)
       --table: first a markdown table of the kernels that differ - registers, scratch, instruction counts of both
       --alias: rename the (mangled) symbols of the SECOND library that match REGEX before comparing, for a kernel template
                that gained a defaulted parameter: its old instantiations carry the default in their names, e.g.
                --alias 'martini_md_step_kernelI(.)Lb(.)ELb(.)ELb0EEE=martini_md_step_kernelI\1Lb\2ELb\3EEE'

Compared PER CODE OBJECT (one per translation unit, in link order), not per library: an fp64 kernel that leaked into the
fp32 unit would hide behind an identical name in a per-library comparison.  For every function symbol of a code object:
  - a hash of its `llvm-objdump -d` text with the address / encoding comment stripped - the whole function, no
    instruction is looked for;
  - for kernels, the metadata the runtime and the occupancy depend on: VGPR, SGPR, LDS bytes, scratch bytes, kernarg size.
Required: the same symbols in every code object, and the same hash and metadata for every symbol.
"""
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from check_exec0_reloads import OBJDUMP, READELF, code_objects  # noqa: E402

FUNC = re.compile(r"^[0-9a-f]+ <(\S+)>:")
META_KEYS = {
    ".vgpr_count": "vgpr",
    ".sgpr_count": "sgpr",
    ".group_segment_fixed_size": "lds",
    ".private_segment_fixed_size": "scratch",
    ".kernarg_segment_size": "kernarg",
}


def functions(elf):
    """{symbol: (sha1 of the disassembly text, instruction count)}"""
    out = subprocess.run([OBJDUMP, "-d", str(elf)], check=True, capture_output=True, text=True).stdout
    funcs, name, h, count = {}, None, None, 0
    for ln in out.split("\n"):
        m = FUNC.match(ln)
        if m:
            if name is not None:
                funcs[name] = (h.hexdigest(), count)
            name, h, count = m.group(1), hashlib.sha1(), 0
        elif name is not None and ln.startswith("\t"):
            h.update(ln.split("//")[0].rstrip().encode() + b"\n")
            count += 1
    if name is not None:
        funcs[name] = (h.hexdigest(), count)
    empty = [n for n, (_, c) in funcs.items() if c == 0]
    if not funcs or empty:  # (another objdump's layout: nothing was hashed, and nothing hashed compares equal)
        raise SystemExit(f"isa_diff: no instructions read for {len(empty)} of {len(funcs)} functions of {elf} (e.g. {empty[:1]}): "
                         "the disassembly is not in the layout this script reads")
    return funcs


def metadata(elf):
    """{kernel symbol: {vgpr, sgpr, lds, scratch, kernarg}} from the code object's notes"""
    notes = subprocess.run([READELF, "--notes", str(elf)], check=True, capture_output=True, text=True).stdout
    out, cur = {}, {}
    for ln in notes.split("\n"):
        t = ln.strip()
        if t.startswith("- .agpr_count:"):
            cur = {}
        key = t.split(":")[0]
        if key in META_KEYS:
            cur[META_KEYS[key]] = int(t.split(":")[1])
        if key == ".symbol":  # (not the last key of a kernel's map: .vgpr_count follows, into the same dict)
            out[t.split(":", 1)[1].strip().strip("'").removesuffix(".kd")] = cur
    short = [n for n, m in out.items() if len(m) != len(META_KEYS)]
    if short or (not out and ".symbol:" in notes):  # (the notes are not in the layout read above)
        raise SystemExit(f"isa_diff: incomplete metadata for {len(short)} of {len(out)} kernels of {elf} (e.g. {short[:1]})")
    return out


def describe(lib, alias=None):
    objs = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, obj in enumerate(code_objects(lib)):
            f = Path(tmp) / f"co{k}.elf"
            f.write_bytes(obj)
            objs.append((functions(f), metadata(f)))
            if alias is not None:
                objs[-1] = tuple({alias[0].sub(alias[1], name): v for name, v in d.items()} for d in objs[-1])
            if set(objs[-1][1]) - set(objs[-1][0]) or (objs[-1][0] and not objs[-1][1]):
                raise SystemExit(f"isa_diff: code object {k} of {lib}: kernels in the notes and functions in the disassembly do not match")
    return objs


def table(a, b):
    """The kernels whose text or metadata differ, one markdown row each (first library -> second), and how many of them
    break what a refactor may not: LDS bytes and kernarg size equal, scratch bytes not above the first library's."""
    names = [n for (fa, _), (fb, _) in zip(a, b) for n in sorted(set(fa) & set(fb))]
    short = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout.split("\n")))
    print("| kernel | VGPR | SGPR | scratch B | instructions | LDS, kernarg |\n|---|---|---|---|---|---|")
    broken = 0
    for k, ((fa, ma), (fb, mb)) in enumerate(zip(a, b)):
        for name in sorted(set(fa) & set(fb)):
            if fa[name] == fb[name] and ma.get(name) == mb.get(name):
                continue
            pa, pb = ma.get(name, {}), mb.get(name, {})
            ok = pa.get("lds") == pb.get("lds") and pa.get("kernarg") == pb.get("kernarg") and pb.get("scratch", 0) <= pa.get("scratch", 0)
            broken += not ok
            cell = lambda key: f"{pa.get(key)} -> {pb.get(key)}" if pa.get(key) != pb.get(key) else f"{pa.get(key)}"
            label = short[name].split("(")[0].replace("void mythos::", "")
            print(f"| `{label}` | {cell('vgpr')} | {cell('sgpr')} | {cell('scratch')} | {fa[name][1]} -> {fb[name][1]} | "
                  f"{cell('lds')}, {cell('kernarg')}{'' if ok else ' **not allowed**'} |")
    return broken


def main():
    want_table = "--table" in sys.argv
    if want_table:
        sys.argv.remove("--table")
    alias = None
    if "--alias" in sys.argv:
        k = sys.argv.index("--alias")
        pattern, repl = sys.argv[k + 1].split("=", 1)
        alias = (re.compile(pattern), repl)
        del sys.argv[k:k + 2]
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    a, b = describe(sys.argv[1]), describe(sys.argv[2], alias)
    if want_table and len(a) == len(b):
        broken = table(a, b)
        print(f"\n{broken} kernel(s) with more scratch, other LDS bytes or another kernarg size")
    bad = 0
    if len(a) != len(b):
        print(f"code objects: {len(a)} against {len(b)}")
        return 1
    total = kernels = 0
    for k, ((fa, ma), (fb, mb)) in enumerate(zip(a, b)):
        for name in sorted(set(fa) | set(fb)):
            where = f"code object {k}: {name[:140]}"
            if name not in fa or name not in fb:
                print(f"{where}\n    only in the {'first' if name in fa else 'second'} library")
                bad += 1
                continue
            total += 1
            if fa[name] != fb[name]:
                print(f"{where}\n    text differs ({fa[name][1]} against {fb[name][1]} instructions)")
                bad += 1
            if ma.get(name) != mb.get(name):
                print(f"{where}\n    metadata {ma.get(name)} against {mb.get(name)}")
                bad += 1
        kernels += len(ma)
        if set(ma) != set(mb):
            print(f"code object {k}: kernel sets differ: {sorted(set(ma) ^ set(mb))[:8]}")
            bad += 1
    steps = sum(1 for fa, _ in a for name in fa if "md_step_kernel" in name)
    print(f"{len(a)} code objects, {total} functions compared ({kernels} kernels with metadata, {steps} md_step_kernel): "
          f"{'IDENTICAL' if bad == 0 else str(bad) + ' difference(s)'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
