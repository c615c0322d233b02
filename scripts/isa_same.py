#!/usr/bin/env python3
r"""Are the kernels of two device .s files the same code, kernel by kernel?
usage: scripts/isa_same.py parent.s tree.s [parent2.s tree2.s ...]

The files come from `hipcc $(HIPFLAGS) --cuda-device-only -S unit.hip` on two trees.  Whole files do
not compare equal after a host-side change (the order of instantiation reorders the kernels), so each
kernel is compared by its mangled name: the instruction text between its label and its .Lfunc_end,
comments dropped and the .LBBn_m labels renumbered in order of first appearance, and its
.amdhsa_kernel block (registers, scratch, LDS, ...).  Exit status 0: the same kernel names on both
sides and every kernel equal; 1 otherwise, with the names that differ.

--rename RE REPL (before the files): the tree's text is rewritten with re.sub(RE, REPL) first, for a
change that gave every kernel a new template argument and so a new mangled name (round 11:
--rename '(sweepk_kernelI\w+)ELb0EEEvNS_' '\1EEEvNS_' drops sweepk_kernel's trailing XF = false).
--new RE: kernels only in the tree whose (rewritten) name matches RE are new instantiations: listed,
not counted as a difference."""
import re
import sys


def kernels(path, rename=None):
    s = open(path).read()
    if rename:
        s = re.sub(rename[0], rename[1], s)
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", s, re.M | re.S):
        name, desc = m.group(1), m.group(2)
        i = s.index("\n" + name + ":") + 1
        j = min(s.index(".Lfunc_end", i), s.index(".amdhsa_kernel", i))  # (the descriptor may stand before .Lfunc_end)
        labels, body = {}, []
        for ln in s[i:j].splitlines():
            ln = ln.split(";", 1)[0].strip()
            if ln:
                body.append(re.sub(r"\.LBB\d+_\d+", lambda t: labels.setdefault(t.group(0), ".L%d" % len(labels)), ln))
        desc = [ln.split(";", 1)[0].strip() for ln in desc.splitlines()]
        out[name] = (body, [ln for ln in desc if ln])
    return out


def main(argv):
    rename = new = None
    while argv and argv[0] in ("--rename", "--new"):
        if argv[0] == "--rename":
            rename, argv = (argv[1], argv[2]), argv[3:]
        else:
            new, argv = argv[1], argv[2:]
    if len(argv) < 2 or len(argv) % 2:
        sys.exit(__doc__)
    bad = 0
    for pa, pb in zip(argv[0::2], argv[1::2]):
        a, b = kernels(pa), kernels(pb, rename)
        for name in sorted(set(b) - set(a)):
            if new and re.search(new, name):
                print("new in %s: %s" % (pb, name))
                del b[name]
        for name in sorted(set(a) ^ set(b)):
            print("only in %s: %s" % (pa if name in a else pb, name))
        diff = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
        for name in diff:
            what = "code" if a[name][0] != b[name][0] else "kernel descriptor"
            print("differs (%s): %s" % (what, name))
        print("%s | %s: %d | %d kernels, %d differ" % (pa, pb, len(a), len(b), len(diff)))
        bad += len(set(a) ^ set(b)) + len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
