#!/usr/bin/env python3
"""Compare two `hipcc --cuda-device-only -S` outputs of one translation unit function by function.

    hipcc <the Makefile's flags> --cuda-device-only -S ls_ivf_subset.hip -o new.s     (and old.s at the other commit)
    tools/kernel_asm_diff.py old.s new.s

A whole-file cmp is of no use: another instantiation order reorders the functions and renumbers their labels. Here a
function is the text from its section directive (`.section .text.<symbol>` for a template instantiation, `.text`
otherwise) to the next function's, the trailing file metadata and the padding behind the last function are cut, and the
label numbers that depend on the function's position (.LBB<n>, .Lfunc_begin<n>, .Lfunc_end<n>, .LJTI<n>, .Ltmp<n>, BB<n>_
in the loop comments, and the column of a label's comment) become a fixed token. Prints the symbol counts, the symbols
only one file has and the bodies that differ; exit status 0 when the sets and every body are identical. It compares text
and looks for no instruction."""
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")
LABEL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+")
PAD = re.compile(r"^(\.LBB#_\d+:) +;", re.M)  # (a label's comment column moves with the digits of <n>)
LOOP = re.compile(r"\bBB\d+(?=_\d)")  # the same numbers in the loop comments ("Header=BB<n>_7", "Parent Loop BB<n>_7")
TRAILER = ("\t.section\t.AMDGPU.gpr_maximums", "\t.amdgpu_metadata")


def functions(path):
    lines = open(path).read().split("\n")
    end = min([i for i, l in enumerate(lines) if l.startswith(TRAILER)] or [len(lines)])
    # (the trap padding behind the file's last function - .text / .p2alignl 6 / .fill 256 - is the file's, not that function's)
    pad = [i - 1 for i, l in enumerate(lines[:end]) if l.startswith("\t.p2alignl 6, ") and lines[i - 1] == "\t.text"]
    end = min(pad + [end])
    starts = [(i - 1, BEGIN.search(l).group(1)) for i, l in enumerate(lines[:end]) if BEGIN.search(l)]
    out = {}
    for (a, sym), (b, _) in zip(starts, starts[1:] + [(end, None)]):
        assert sym not in out and re.match(r"\t\.(text$|section\t\.text\.)", lines[a]), (path, sym, lines[a])
        out[sym] = PAD.sub(r"\1 ;", LOOP.sub("BB#", LABEL.sub(r".\1#", "\n".join(lines[a:b]))))
    return out


def main(old, new):
    fo, fn = functions(old), functions(new)
    only = sorted(set(fo) ^ set(fn))
    differ = sorted(s for s in set(fo) & set(fn) if fo[s] != fn[s])
    for s in only:
        print("only in", old if s in fo else new, ":", s)
    for s in differ:
        print("body differs:", s)
    same = len(set(fo) & set(fn)) - len(differ)
    print(f"{old}: {len(fo)} functions, {new}: {len(fn)} functions, {same} of {len(fo)} bodies identical")
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
