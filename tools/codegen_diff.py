#!/usr/bin/env python3
"""Compares the gfx950 device assembly of two csrc trees, function by function (no GPU needed).

    tools/codegen_diff.py PARENT_CSRC THIS_CSRC [unit ...] [--json OUT] [--show N] [-j JOBS]

Every .hip / .cpp unit (default: all of THIS_CSRC) of both trees is compiled with the flags of tests/codegen_util.py, the `__hip_cuid_` lines are
dropped, and each function gets one verdict:
    identical   the same lines and the same kernel descriptor block
    same code   other lines, but the same multiset of instruction mnemonics and an equal kernel descriptor block: the `.amdhsa_` lines and the metadata's vgpr / sgpr /
                spill counts, private and group segment sizes (what renamed registers, moved scratch slots or two swapped instructions leave alone)
    differs     anything else, a function that only one tree has included
The exit status is 1 if any function differs."""
import argparse
import collections
import concurrent.futures
import difflib
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from codegen_util import FLAGS  # noqa: E402

META_KEYS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
Function = collections.namedtuple("Function", "lines mnemonics descriptor")


def functions(text):
    """{name: Function} of one assembly listing."""
    lines = [l for l in text.split("\n") if "__hip_cuid_" not in l]
    meta, cur = {}, None                       # the metadata's counts per kernel: entries of `amdhsa.kernels:`, each opened by "  - "
    start = next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines))
    for l in lines[start + 1:]:
        if not l.startswith("  "):
            break
        if l.startswith("  - "):
            cur = {}
        m = re.match(r"^(?:  - |    )(\.\w+):\s*(\S+)\s*$", l)
        if m and m.group(1) == ".name":
            meta[m.group(2)] = cur
        elif m and m.group(1) in META_KEYS:
            cur[m.group(1)] = m.group(2)
    out, names, i = {}, set(), 0
    while i < len(lines):
        m = re.match(r"^\s+\.type\s+(\S+),@function", lines[i])
        if m:
            names.add(m.group(1))
        m = re.match(r"^([\w.$]+):", lines[i])
        if m and m.group(1) in names:
            end = next(j for j in range(i, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[j]))
            body = lines[i:end]
            mnem = collections.Counter(x.split()[0] for x in body if re.match(r"^\s+[a-z]", x))
            desc = [x.strip() for x in body if x.strip().startswith(".amdhsa_")] + ["%s %s" % kv for kv in sorted(meta.get(m.group(1), {}).items())]
            out[m.group(1)] = Function(body, mnem, desc)
            i = end
        i += 1
    return out


def verdict(a, b):
    if a is None or b is None:
        return "differs"
    if a.descriptor != b.descriptor or a.mnemonics != b.mnemonics:
        return "differs"
    return "identical" if a.lines == b.lines else "same code"


def compare_listings(parent_text, this_text):
    """{function: verdict} of two listings of one unit."""
    pa, th = functions(parent_text), functions(this_text)
    return {name: verdict(pa.get(name), th.get(name)) for name in sorted(set(pa) | set(th))}


def first_differences(parent_text, this_text, name, n):
    """Why a function differs (the mnemonics one side has more of, or the descriptor), then the first n differing lines."""
    pa, th = functions(parent_text).get(name), functions(this_text).get(name)
    if pa is None or th is None:
        return ["only in " + ("this" if pa is None else "parent")]
    why = ["%+d %s" % (th.mnemonics[m] - pa.mnemonics[m], m) for m in sorted(set(pa.mnemonics) | set(th.mnemonics)) if th.mnemonics[m] != pa.mnemonics[m]]
    why += [l for l in difflib.unified_diff(pa.descriptor, th.descriptor, n=0, lineterm="") if l[0] in "+-" and l[:3] not in ("---", "+++")]
    diff = difflib.unified_diff(pa.lines, th.lines, n=0, lineterm="")
    return ["(" + ", ".join(why) + ")"] + [l for l in diff if not l.startswith(("@@", "---", "+++"))][:n]


def compile_unit(csrc, unit, out):
    r = subprocess.run(["hipcc", *FLAGS, unit, "-o", out], capture_output=True, text=True, cwd=csrc)
    if r.returncode:
        sys.exit("%s of %s does not compile:\n%s" % (unit, csrc, r.stderr))
    return open(out).read()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_csrc")
    ap.add_argument("this_csrc")
    ap.add_argument("units", nargs="*")
    ap.add_argument("--json", help="write the table to this file")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N differing lines of every function that differs")
    ap.add_argument("-j", "--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    units = args.units or sorted(f for f in os.listdir(args.this_csrc) if f.endswith((".hip", ".cpp")))
    table, differs = {}, 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        jobs = {(u, side): pool.submit(compile_unit, os.path.abspath(csrc), u, os.path.join(tmp, "%s.%s.s" % (u, side)))
                for u in units for side, csrc in (("parent", args.parent_csrc), ("this", args.this_csrc))}
        for u in units:
            pa, th = jobs[u, "parent"].result(), jobs[u, "this"].result()
            table[u] = compare_listings(pa, th)
            counts = collections.Counter(table[u].values())
            print("%-20s %4d functions: %s" % (u, len(table[u]), ", ".join("%d %s" % (counts[v], v) for v in ("identical", "same code", "differs") if counts[v]) or "-"))
            for name, v in table[u].items():
                if v != "identical":
                    print("    %-10s %s" % (v, name))
                if v == "differs":
                    differs += 1
                    for l in first_differences(pa, th, name, args.show) if args.show else []:
                        print("        " + l)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"flags": FLAGS, "units": table}, f, indent=1, sort_keys=True)
            f.write("\n")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
