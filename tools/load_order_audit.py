#!/usr/bin/env python3
"""Audit of the request order of quantize_tiled8_kernel's full-workgroup path (csrc/mq_quantize.hip; DESIGN 4.1 "request order").
On cold caches the kernel's time is the number of dependent round trips that stand in a row, and hipcc reorders requests freely: a
load whose use is conditional is sunk into the branch, behind the grid values' wait and the divide, and waited for with vmcnt(0);
a kernel argument used only in the tail is read there, behind the barrier.
usage: load_order_audit.py file.s ...   (hipcc -S --cuda-device-only output of mq_quantize.hip).  For every instantiation
quantize_tiled8_kernel<V, HAS_SUM, GRPS> the full-workgroup path is the entry block (up to the first branch) followed by the text
between the source's two comment markers `mq-full-path-begin` / `mq-full-path-end`.  On it:
  LOADS    exactly 2 V global_load_dwordx4, all in front of the first s_waitcnt that names vmcnt
  WAIT     that first wait is not vmcnt(0) for V > 1 (the conversions follow the loads one by one)
  GRID     no s_waitcnt that names lgkmcnt stands between the first and the last of these loads (the grid values' wait, and the divide
           behind it, follow the last request)
  KERNARG  no read of the kernel-argument segment (s_load off s[0:1], the kernarg pointer, until the code reuses the pair) follows the
           first vector load, anywhere in the function
A violation prints a line `<file>:<line> LOADS|WAIT|GRID|KERNARG <kernel>: <what>`; the last line counts kernels and violations."""
import re
import sys

KERNEL = re.compile(r"^(_ZN2mq22quantize_tiled8_kernelILi(\d)ELb([01])ELi(\d)E\w*):")
BEGIN, END = "mq-full-path-begin", "mq-full-path-end"


def _instr(line):
    """the instruction text of a line, or '' for labels, directives, comments and blank lines"""
    t = line.split(";")[0].strip()
    return "" if (not t or t.endswith(":") or t.startswith(".")) else t


def _vm_wait(t):
    """the vmcnt value an s_waitcnt waits for, or None when it leaves vmcnt alone (a bare immediate waits for everything)"""
    if not t.startswith("s_waitcnt"):
        return None
    m = re.search(r"vmcnt\((\d+)\)", t)
    if m:
        return int(m.group(1))
    return 0 if re.match(r"^s_waitcnt\s+(0x[0-9a-f]+|\d+)$", t) else None


def _writes_kernarg_ptr(t):
    m = re.match(r"^s_\w+\s+(s\d+|s\[\d+:\d+\])\s*,", t)
    if not m or t.startswith(("s_cmp", "s_bitcmp", "s_waitcnt", "s_cbranch", "s_branch")):
        return False
    d = m.group(1)
    lo, hi = (int(d[1:]),) * 2 if "[" not in d else map(int, d[2:-1].split(":"))
    return lo <= 1 and hi >= 0


def audit_kernel(name, V, lines, first, last):
    """violations [(line number, kind, text)] of one function: lines[first:last]"""
    bad = []
    begin = next((n for n in range(first, last) if BEGIN in lines[n]), None)
    end = next((n for n in range(first, last) if END in lines[n]), None)
    if begin is None or end is None or end < begin:
        return [(first + 1, "LOADS", "no full-workgroup path: the markers %s / %s are missing" % (BEGIN, END))]
    branch = next((n for n in range(first, last) if _instr(lines[n]).startswith(("s_cbranch", "s_branch"))), last)
    entry_end = min(branch, begin)
    path = list(range(first, entry_end + 1)) + list(range(max(begin, entry_end + 1), end + 1))
    loads = [n for n in path if _instr(lines[n]).startswith("global_load_dwordx4")]
    waits = [(n, _vm_wait(_instr(lines[n]))) for n in path if _vm_wait(_instr(lines[n])) is not None]
    if len(loads) != 2 * V:
        bad.append((begin + 1, "LOADS", "%d global_load_dwordx4 on the path, want %d" % (len(loads), 2 * V)))
    if not waits:
        bad.append((begin + 1, "WAIT", "no vmcnt wait on the path"))
    else:
        n0, c0 = waits[0]
        late = [n for n in loads if n > n0]
        if late:
            bad.append((late[0] + 1, "LOADS", "%d of the loads stand behind the first vmcnt wait (line %d)" % (len(late), n0 + 1)))
        if V > 1 and c0 == 0:
            bad.append((n0 + 1, "WAIT", "the first vmcnt wait is vmcnt(0): the first conversion waits for every load"))
    if loads:
        early = [n for n in path if loads[0] < n < loads[-1] and re.match(r"^s_waitcnt\b.*lgkmcnt", _instr(lines[n]))]
        if early:
            bad.append((early[0] + 1, "GRID", "a scalar wait stands in front of %d of the loads" % len([n for n in loads if n > early[0]])))
    # kernel-argument reads, in text order: s[0:1] is the kernarg pointer until something overwrites it
    first_load = next((n for n in range(first, last) if _instr(lines[n]).startswith(("global_load", "buffer_load", "flat_load"))), last)
    for n in range(first, last):
        t = _instr(lines[n])
        if n > first_load and re.match(r"^s_load_dword\w*\s+\S+\s+s\[0:1\]\s*,", t):
            bad.append((n + 1, "KERNARG", "a kernel argument is read behind the first vector load (line %d): %s" % (first_load + 1, t)))
        if _writes_kernarg_ptr(t):
            break
    return bad


def audit(path):
    """(number of kernels, [report lines]) of one assembly file"""
    lines = open(path).read().split("\n")
    starts = [(n, KERNEL.match(l)) for n, l in enumerate(lines) if KERNEL.match(l)]
    out = []
    for n, m in starts:
        last = next((k for k in range(n, len(lines)) if lines[k].startswith(".Lfunc_end")), len(lines))
        V, has_sum, grps = int(m.group(2)), int(m.group(3)), int(m.group(4))
        for ln, kind, what in audit_kernel(m.group(1), V, lines, n, last):
            out.append("%s:%d %s quantize_tiled8_kernel<%d, %s, %d>: %s" % (path.split("/")[-1], ln, kind, V, "true" if has_sum else "false", grps, what))
    return len(starts), out


if __name__ == "__main__":
    for p in sys.argv[1:]:
        count, report = audit(p)
        for line in report:
            print(line)
        print(p.split("/")[-1], "quantize_tiled8_kernel instantiations", count, "request-order violations", len(report))
