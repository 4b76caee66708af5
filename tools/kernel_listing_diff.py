"""Which kernels of a device-only assembly listing differ from another build's: the check that a source change reached only the kernels it meant to.

    hipcc --offload-arch=gfx950 <flags of mosfhet_amd/build.py> --cuda-device-only -S -o /tmp/parent.s mosfhet_amd/csrc/capi.hip     (on the parent commit)
    hipcc --offload-arch=gfx950 <flags of mosfhet_amd/build.py> --cuda-device-only -S -o /tmp/new.s mosfhet_amd/csrc/capi.hip        (on the change)
    python tools/kernel_listing_diff.py /tmp/parent.s /tmp/new.s [name filter] [--where]

--where: for every differing kernel, the differing line ranges of the parent side (lines of the normalised text, counted from the kernel's label), the kernel's
loops -- a backward branch to a label at least 500 lines earlier: the step loop of a bootstrap kernel, not a poll --, whether a difference falls inside one, and
the .amdhsa_* resource lines that changed (registers, LDS, scratch).
A kernel whose loops are untouched runs the parent's instructions in every step; only its prologue or epilogue moved.

Compares, kernel by kernel, the text from the kernel's label to the end of its .amdhsa_kernel block (instructions and resources) after dropping what differs
between any two builds: comments, .loc / .file / .ident lines, the __hip_cuid_* symbol and the function index inside local labels (.LBB<n>_).  Text and
nothing else.  Exit status 0: same kernels on both sides, none differs.
"""
import difflib
import re
import subprocess
import sys

_DROP = re.compile(r"\.(loc|file|ident)\b")
_LOCAL = re.compile(r"\.L(func_begin|func_end|[A-Za-z]+(?=\d+_\d))\d+")   # .LBB<n>_<m> -> .LBB_<m>, .Lfunc_end<n> -> .Lfunc_end
_CUID = re.compile(r"__hip_cuid_\w+")


def _normalise(line):
    line = line.split(";", 1)[0].strip()
    if not line or _DROP.match(line):
        return None
    return _CUID.sub("__hip_cuid", _LOCAL.sub(r".L\1", " ".join(line.split())))


def kernels(text):
    """{mangled name: normalised lines from the kernel's label to .end_amdhsa_kernel}, in listing order"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {}, None
    for raw in text.split("\n"):
        if cur is None:
            label = raw.split(";", 1)[0].rstrip()   # "name:    ; @name"
            if label.endswith(":") and label[:-1] in names:
                cur = out.setdefault(label[:-1], [])
            continue
        line = _normalise(raw)
        if line is not None:
            cur.append(line)
        if line == ".end_amdhsa_kernel":
            cur = None
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    except OSError:
        res = []
    return dict(zip(names, res)) if len(res) >= len(names) else {n: n for n in names}


_BRANCH = re.compile(r"s_c?branch\w*\s+(\S+)$")
LOOP_MIN = 500   # a backward branch over fewer lines is a poll or a short inner loop, not a step loop


def loops(lines, min_len=LOOP_MIN):
    """[(first, last)] 1-based line ranges from a label to a backward branch to it at least min_len lines further down"""
    label = {line[:-1]: i for i, line in enumerate(lines) if line.endswith(":")}
    out = []
    for i, line in enumerate(lines):
        m = _BRANCH.match(line)
        if m and i - label.get(m.group(1), i) >= min_len:
            out.append((label[m.group(1)] + 1, i + 1))
    return out


def where(a, b, min_len=LOOP_MIN):
    """(differing 1-based line ranges of the parent side a -- an insertion is the empty range in front of its line --, a's loops, those of the ranges that touch a loop)"""
    ops = difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
    ranges = [(i1 + 1, i2) for tag, i1, i2, _, _ in ops if tag != "equal"]
    lps = loops(a, min_len)
    def touches(s, e, lo, hi):
        return lo < s <= hi if e < s else (s <= hi and e >= lo)
    inside = [r for r in ranges if any(touches(*r, *lp) for lp in lps)]
    return ranges, lps, inside


def compare(parent, new, filt="", show_where=False, loop_min=LOOP_MIN):
    """(report lines, same?) for two listings' texts"""
    a, b = kernels(parent), kernels(new)
    dm = demangle(sorted(set(a) | set(b)))
    if filt:
        a = {n: v for n, v in a.items() if filt in dm[n]}
        b = {n: v for n, v in b.items() if filt in dm[n]}
    report = ["kernels: %d in the parent listing, %d in the new one" % (len(a), len(b))]
    only_a, only_b = [n for n in a if n not in b], [n for n in b if n not in a]
    for n in only_a:
        report.append("only in the parent listing: %s" % dm[n])
    for n in only_b:
        report.append("only in the new listing: %s" % dm[n])
    differ = [n for n in a if n in b and a[n] != b[n]]
    report.append("kernels that differ: %d" % len(differ))
    for n in differ:
        at = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
        report.append("  %s" % dm[n])
        report.append("    line %d of %d / %d:  parent: %s" % (at + 1, len(a[n]), len(b[n]), a[n][at] if at < len(a[n]) else "<end>"))
        report.append("    %s     new: %s" % (" " * len("line %d of %d / %d:" % (at + 1, len(a[n]), len(b[n]))), b[n][at] if at < len(b[n]) else "<end>"))
        if show_where:
            ranges, lps, inside = where(a[n], b[n], loop_min)
            fmt = lambda rs: ", ".join("%d-%d" % r if r[1] >= r[0] else "before %d" % r[0] for r in rs) or "none"
            report.append("    differing parent lines: %s" % fmt(ranges))
            report.append("    loops (a backward branch over %d lines or more): %s" % (loop_min, fmt(lps)))
            report.append("    differences inside a loop: %s" % fmt(inside))
            ra, rb = ({line.split()[0]: line for line in k if line.startswith(".amdhsa_")} for k in (a[n], b[n]))
            report.append("    resource lines: %s" % (", ".join("%s -> %s" % (ra[k], rb.get(k, "<none>").split()[-1]) for k in ra if ra[k] != rb.get(k)) or "same"))
    if not a:
        report.append("no kernel found in the parent listing")
    return report, bool(a) and not (only_a or only_b or differ)


def main():
    args = [x for x in sys.argv[1:] if x != "--where"]
    if len(args) < 2:
        sys.exit(__doc__)
    with open(args[0]) as fa, open(args[1]) as fb:
        report, same = compare(fa.read(), fb.read(), args[2] if len(args) > 2 else "", show_where="--where" in sys.argv)
    print("\n".join(report))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
