#!/usr/bin/env python3
"""Per-kernel fingerprint of the gfx950 instruction stream of a kernel source.

    python scripts/isa_stream.py native/kernels/gemm_mxfp8.hip [extra hipcc flags]
    python scripts/isa_stream.py native/kernels/gemm_mxfp8.hip --diff OTHER.s
    python scripts/isa_stream.py native/kernels/gemm_mxfp8.hip --save NEW.s
    python scripts/isa_stream.py native/kernels/gemm_bf16_layouts.hip --diff OTHER.s --by-name

Compiles SOURCE with the Makefile's HIPFLAGS plus ``--cuda-device-only -S`` (a
``.s`` file is read as it is) and prints, for every kernel in file order, its
name, the register / LDS / scratch / spill metadata and the SHA-256 of its
normalised instruction stream: the text between the kernel's label and its
``.Lfunc_end``, without comments, assembler directives, blank lines, label
definitions and trailing ``; ...`` remarks.  Branch operands keep their label
names, so two sources compare equal only with their kernels in the same order;
``--by-name`` drops the function number from those labels (``.LBB<f>_<n>``
becomes ``.LBB_<n>``) and compares kernels by name alone, for a change that
moves a template's first point of instantiation: it then lists the kernels
whose position in the file changed.

A refactor that must not move an instruction shows it by equal hashes against
the listing of the parent commit's source; ``--diff`` prints where two
listings part.  ``--vector-sequence`` adds the hash of the mnemonics alone with
scalar ALU and scalar moves dropped (``s_waitcnt`` keeps its operand): equal
there and unequal above means the difference is scalar arithmetic or register
numbering.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
             "private_segment_fixed_size", "group_segment_fixed_size")
# scalar instructions that are neither ALU nor moves
SCALAR_KEPT = ("s_waitcnt", "s_barrier", "s_nop", "s_branch", "s_cbranch", "s_endpgm", "s_load",
               "s_setprio", "s_sleep")


def makefile_hipflags() -> list[str]:
    text = open(os.path.join(REPO, "Makefile")).read().replace("\\\n", " ")
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M))
    flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)].strip(), var["HIPFLAGS"])
    return [f if not f.startswith("-Inative") else "-I" + os.path.join(REPO, f[2:])
            for f in flags.split()]


def listing(source: str, extra: list[str], save: str | None) -> str:
    if source.endswith(".s"):
        return open(source).read()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = save or os.path.join(tmp, "k.s")
        subprocess.run([hipcc, *makefile_hipflags(), *extra, "--cuda-device-only", "-S", source,
                        "-o", out], check=True)
        return open(out).read()


def kernels(asm: str, by_name: bool = False) -> list[tuple[str, dict[str, str], list[str]]]:
    """(name, metadata, normalised stream) of every kernel, in file order."""
    meta: dict[str, dict[str, str]] = {}
    entry: dict[str, str] = {}
    for line in asm[asm.find("amdhsa.kernels:"):].splitlines():
        if line.startswith("  - "):
            entry = {}
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)$", line)
        if m:
            entry[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = entry
    lines = asm.splitlines()
    found = []
    for i, line in enumerate(lines):
        m = re.match(r"([A-Za-z_][\w$.]*):", line)
        if not m or m.group(1) not in meta:
            continue
        stream = []
        for body in lines[i + 1:]:
            if body.startswith(".Lfunc_end"):
                break
            body = body.split(";", 1)[0].strip()
            if body and not body.startswith(".") and not re.fullmatch(r"[\w$.]+:", body):
                body = re.sub(r"\s+", " ", body)
                stream.append(re.sub(r"\.LBB\d+_", ".LBB_", body) if by_name else body)
        found.append((m.group(1), meta[m.group(1)], stream))
    return found


def vector_sequence(stream: list[str]) -> list[str]:
    seq = []
    for ins in stream:
        op = ins.split(" ", 1)[0]
        if op.startswith("s_") and not op.startswith(SCALAR_KEPT):
            continue
        seq.append(ins if op == "s_waitcnt" else op)
    return seq


def digest(lines: list[str]) -> str:
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def demangle(names: list[str]) -> list[str]:
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    try:
        out = subprocess.run([filt, *names], check=True, capture_output=True, text=True).stdout
        short = [re.sub(r"\(anonymous namespace\)::|\(.*", "", n) for n in out.splitlines()]
        return short if len(short) == len(names) else names
    except (OSError, TypeError, subprocess.CalledProcessError):
        return names


def first_difference(a: list[str], b: list[str], context: int) -> str:
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    differing = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    rows = [f"    {len(a)} / {len(b)} lines, {differing} differ by position, first at {n}"]
    for i in range(n, min(n + context, max(len(a), len(b)))):
        rows.append(f"    {i:6d}  {a[i] if i < len(a) else '-':<60}| {b[i] if i < len(b) else '-'}")
    return "\n".join(rows)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("source", help="kernel source (.hip) or an assembly listing (.s)")
    ap.add_argument("--diff", metavar="OTHER.s", help="compare every kernel with this listing")
    ap.add_argument("--save", metavar="OUT.s", help="keep the compiled listing")
    ap.add_argument("--vector-sequence", action="store_true",
                    help="also hash the mnemonics without scalar ALU and scalar moves")
    ap.add_argument("--by-name", action="store_true",
                    help="labels without their function number; kernels may change position")
    ap.add_argument("--context", type=int, default=8, help="lines shown by --diff")
    args, extra = ap.parse_known_args()
    mine = kernels(listing(args.source, extra, args.save), args.by_name)
    other = kernels(open(args.diff).read(), args.by_name) if args.diff else []
    theirs = {n: (m, s) for n, m, s in other}
    same = not args.diff or {n for n, _, _ in mine} == set(theirs)
    for name in set(theirs) - {n for n, _, _ in mine}:
        print(f"DIFF: {name} only in {args.diff}")
    if args.diff and [n for n, _, _ in mine] != [n for n, _, _ in other]:
        moved = [n for i, (n, _, _) in enumerate(mine) if i >= len(other) or other[i][0] != n]
        print(f"kernel order differs from {args.diff} at {len(moved)} positions"
              + ("" if args.by_name else " (branch labels carry the function number: --by-name)"))
        same = same and args.by_name
    for (name, meta, stream), shown in zip(mine, demangle([n for n, _, _ in mine])):
        print(shown)
        print("  " + " ".join(f"{k}={meta.get(k, '?')}" for k in META_KEYS))
        print(f"  stream {len(stream)} lines sha256 {digest(stream)}")
        if args.vector_sequence:
            seq = vector_sequence(stream)
            print(f"  vector sequence {len(seq)} lines sha256 {digest(seq)}")
        if args.diff:
            if name not in theirs:
                print("  DIFF: not in " + args.diff)
                same = False
                continue
            ometa, ostream = theirs[name]
            moved = [k for k in META_KEYS if meta.get(k) != ometa.get(k)]
            if moved:
                print("  DIFF metadata: " + " ".join(f"{k}={meta.get(k)}/{ometa.get(k)}" for k in moved))
            if stream != ostream:
                print("  DIFF stream:\n" + first_difference(stream, ostream, args.context))
                if args.vector_sequence:
                    a, b = vector_sequence(stream), vector_sequence(ostream)
                    print("  vector sequence " + ("identical" if a == b else
                                                  "DIFF:\n" + first_difference(a, b, args.context)))
            same = same and not moved and stream == ostream
            if not moved and stream == ostream:
                print("  identical to " + args.diff)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
