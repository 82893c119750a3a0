"""Compare the gfx950 device code of two builds, kernel by kernel (for refactors that must leave every kernel as it was).

    python tools/device_code_diff.py <objdir_a> <objdir_b> [--allow-removed REGEX]

For each object `<source>.hip.<hash>.o` present in both directories (the hash differs between builds, so objects
are paired by source name) the code objects are disassembled (tools/isa_hazards.py) and the functions compared by
their exact mangled names: functions only in a, only in b, and in both with differing instruction lists
(mnemonic + operands, branch targets as positions in the function).  The bytes of two code objects differ even when their text is equal (the compilation-unit
id is in them), hence the comparison on disassembly.  Exit status 1 on any difference except functions missing
from b whose name matches --allow-removed."""
from __future__ import annotations

import argparse
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_hazards import disassemble, parse  # noqa: E402


def objects(objdir: str) -> dict:
    """source name -> object path"""
    out = {}
    for path in sorted(glob.glob(os.path.join(objdir, "*.hip.*.o"))):
        out[os.path.basename(path).rsplit(".", 2)[0]] = path
    return out


def functions(obj: str) -> dict:
    """name -> [(mnemonic, operands)], a branch target given as the target's index in the function (the
    disassembler numbers its labels through the whole object, so their names shift when a function is removed)"""
    out = {}
    for name, ins, labels in parse(disassemble(obj)):
        out[name] = [(mn, f"@{labels[ops.strip()]}" if ops.strip() in labels else ops) for mn, ops in ins]
    return out


def main(argv) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("objdir_a")
    ap.add_argument("objdir_b")
    ap.add_argument("--allow-removed", metavar="REGEX", help="functions that may be missing from b")
    args = ap.parse_args(argv)
    allowed = re.compile(args.allow_removed) if args.allow_removed else None
    a, b = objects(args.objdir_a), objects(args.objdir_b)
    bad = 0
    for src in sorted(set(a) ^ set(b)):
        bad += 1
        print(f"{src}: only in {'a' if src in a else 'b'} (not compared)")
    for src in sorted(set(a) & set(b)):
        fa, fb = functions(a[src]), functions(b[src])
        only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
        differ = sorted(n for n in set(fa) & set(fb) if fa[n] != fb[n])
        same = len(set(fa) & set(fb)) - len(differ)
        print(f"{src}: {len(fa)} functions in a, {len(fb)} in b, {same} identical, {len(differ)} differ, "
              f"{len(only_a)} only in a, {len(only_b)} only in b")
        for n in only_a:
            ok = allowed is not None and allowed.search(n) is not None
            bad += not ok
            print(f"  only in a{' (allowed)' if ok else ''}: {n}")
        for n in only_b:
            bad += 1
            print(f"  only in b: {n}")
        for n in differ:
            bad += 1
            first = next((i for i, (x, y) in enumerate(zip(fa[n], fb[n])) if x != y), min(len(fa[n]), len(fb[n])))
            print(f"  differs: {n}: {len(fa[n])} vs {len(fb[n])} instructions, first difference at [{first}]")
    print(f"{len(set(a) & set(b))} objects compared, {bad} differences outside --allow-removed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
