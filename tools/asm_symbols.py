#!/usr/bin/env python3
"""Per-symbol comparison of the gfx950 assembly of two trees: `make -C software-raytracer_amd/csrc asm` in each
tree leaves build/asm/*gfx950*.s; this prints, for every function of either listing, its instruction-line count and a SHA-256 of
its text with comments dropped and local labels (.LBB<n>_<m>, .Ltmp<n>, .LJTI<n>_<m>) renumbered in order of appearance, for both
trees, and `same`, `DIFFERS`, `new` or `gone`; the last line counts them.  Exit status 1 when a function of the first tree differs
or is gone.

    python tools/asm_symbols.py PARENT_TREE/build/asm THIS_TREE/build/asm > profiles/probe_tail/probe_tail_asm.txt"""
import glob
import hashlib
import re
import sys


def functions(directory):
    out, cur = {}, None
    for line in open(glob.glob(directory + "/*gfx950*.s")[0]):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"^\s*\.size", line):
            cur = None
            continue
        if re.match(r"^\s*\.Lfunc_end", line):
            continue
        text = line.split(";")[0].rstrip()
        if text.strip():
            out[cur].append(text)
    return out


def digest(lines):
    names = {}

    def renumber(m):
        return names.setdefault(m.group(0), "L%d" % len(names))

    body = "\n".join(re.sub(r"\.LBB\d+_\d+|\.Ltmp\d+|\.LJTI\d+_\d+", renumber, l) for l in lines)
    return hashlib.sha256(body.encode()).hexdigest()[:16]


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    counts = dict(same=0, DIFFERS=0, new=0, gone=0)
    for name in sorted(set(a) | set(b)):
        da, db = (digest(a[name]) if name in a else "-"), (digest(b[name]) if name in b else "-")
        verdict = "new" if name not in a else "gone" if name not in b else "same" if da == db else "DIFFERS"
        counts[verdict] += 1
        print("%-8s %6s %-16s %6s %-16s %s" % (verdict, len(a.get(name, ())) or "-", da, len(b.get(name, ())) or "-", db, name))
    print("first tree %d functions, second %d: %d same, %d differ, %d new, %d gone" % (len(a), len(b), counts["same"], counts["DIFFERS"], counts["new"], counts["gone"]))
    return 1 if counts["DIFFERS"] or counts["gone"] else 0


if __name__ == "__main__":
    sys.exit(main())
