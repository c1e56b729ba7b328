#!/usr/bin/env python3
"""Compares two device-only assembly files of rl_api.hip kernel by kernel.

    hipcc $(FLAGS of csrc/Makefile) -DRL_BUILD_ID='"x"' --cuda-device-only -S -o a.s rl_api.hip     (in each tree's csrc/)
    tools/kernel_isa_diff.py a.s b.s

Per kernel symbol (every .amdhsa_kernel of either file, mangled or not): identical, or the number of instruction lines that differ
out of the total, after dropping comments, directives and blank lines and renumbering the .LBB labels, and the .Lpost_getpc labels of
long branches (numbered through the whole file, so a kernel added in front moves them), in order of appearance; and
the metadata figures (VGPRs, SGPRs, spilled SGPRs, scratch bytes) of both side by side.  Exit status 0 whatever it finds: it
reports, it does not judge.  No GPU needed."""
import difflib
import re
import sys


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    out = {}
    for name in names:
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M).group(1)
        labels, lines = {}, []
        for line in body.splitlines():
            line = line.split(";")[0].strip() if ";;#ASM" not in line else ""
            if not line or (line.startswith(".") and not line.startswith(".LBB")):
                continue
            lines.append(line)
        for line in lines:   # labels numbered by first appearance, definition or use
            for lab in re.findall(r"\.LBB\d+_\d+|\.Lpost_getpc\d+", line):
                labels.setdefault(lab, ".L%d" % len(labels))
        lines = [re.sub(r"\.LBB\d+_\d+|\.Lpost_getpc\d+", lambda m: labels[m.group(0)], l) for l in lines]
        meta = re.search(r"^\s+\.name:\s+%s\n(.*?)^\s+\.wavefront_size" % re.escape(name), text, re.S | re.M).group(1)
        figure = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))
        out[name] = (lines, (figure("vgpr_count"), figure("sgpr_count"), figure("sgpr_spill_count"), figure("private_segment_fixed_size")))
    return out


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    print("# kernel_isa_diff: A = %s, B = %s" % (a_path, b_path))
    print("# per kernel: verdict; (VGPRs, SGPRs, spilled SGPRs, scratch bytes) of A -> of B")
    same = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%-9s %s" % ("only in " + ("A" if name in a else "B"), name))
            continue
        (la, ma), (lb, mb) = a[name], b[name]
        if la == lb:
            verdict = "identical (%d lines)" % len(la)
            same += 1
        else:
            sm = difflib.SequenceMatcher(None, la, lb, autojunk=False)
            changed = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")
            verdict = "DIFFERS: %d of %d / %d lines" % (changed, len(la), len(lb))
        print("%s\n    %s; %s -> %s%s" % (name, verdict, ma, mb, "" if ma == mb else "  (figures differ)"))
    print("# %d of %d kernels identical" % (same, len(set(a) | set(b))))


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
