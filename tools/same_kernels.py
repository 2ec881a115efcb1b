#!/usr/bin/env python3
"""Do two builds hold the same kernels? Compares gfx950 assembly (hipcc --offload-device-only -S; build.device_assembly),
kernel by kernel: a change that only moves code between translation units, or is not meant to reach the compiler's
output, leaves every function of namespace jg with the same instructions and the same register and scratch use.

    python tools/same_kernels.py before.s [more.s ...] -- after.s [more.s ...]

A function is compared under its mangled name (_ZN2jg...), whichever file of its side holds it: its text without comments,
blank lines and .loc / .file / .cfi lines, with the numbers of local labels (.LBB<f>_<n>, .Ltmp<n>, .Lfunc_*<n>) replaced,
and its `.set <name>.num_vgpr`, `.num_sgpr` (`.numbered_sgpr`) and `.private_seg_size` values. Prints the names that differ or that one
side lacks; exit status 1 if there is any."""
import re
import sys

_LABEL = re.compile(r"\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?")
_SET = re.compile(r"^\s*\.set (_ZN2jg\S+)\.(num_vgpr|num_sgpr|numbered_sgpr|private_seg_size), (.*)$")
_FUNC = re.compile(r"^\s*\.type\s+(_ZN2jg\S+),@function")


def kernels(paths):
    """{mangled name: (instruction lines, {resource: value})} over the files of one side."""
    out = {}
    for path in paths:
        name, funcs = None, set()
        for ln in open(path):
            m = re.match(r"^(_ZN2jg\S*):", ln)
            s = _SET.match(ln)
            if _FUNC.match(ln):
                funcs.add(_FUNC.match(ln).group(1))
            elif m and m.group(1) in funcs:
                name = m.group(1)
                assert name not in out, "%s: defined twice on one side" % name
                out[name] = ([], {})
            elif name is not None and ln.startswith(".Lfunc_end"):
                name = None
            elif name is not None:
                code = _LABEL.sub(lambda x: ".L%sN%s" % (x.group(1), "_N" if x.group(2) else ""), ln.split(";")[0].rstrip())
                if code.strip() and not code.strip().startswith((".loc", ".file", ".cfi")):
                    out[name][0].append(code)
            elif s and s.group(1) in out:
                out[s.group(1)][1][s.group(2)] = s.group(3).strip()
    return out


def main(argv):
    if "--" not in argv:
        sys.exit(__doc__)
    a, b = kernels(argv[:argv.index("--")]), kernels(argv[argv.index("--") + 1:])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only %s: %s" % ("before" if name in a else "after", name))
        elif a[name][0] != b[name][0]:
            print("instructions differ: %s" % name)
        elif a[name][1] != b[name][1]:
            print("registers / scratch differ: %s: %s -> %s" % (name, a[name][1], b[name][1]))
        else:
            continue
        bad += 1
    print("%d of %d functions equal, %d differ or are missing" % (len(set(a) | set(b)) - bad, len(set(a) | set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
