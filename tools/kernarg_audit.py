#!/usr/bin/env python3
"""Audit of the kernel-argument preload of the headline step's two kernels (DESIGN 4.1 / 4.2 "kernel arguments"): gfx950 delivers the
first 14 dwords of scalar parameters in user SGPRs at wave launch when the code object asks for it (build.KERNARG_PRELOAD), so a wave
need not open with a cold read of its own kernel-argument segment.  hipcc puts a backward-compatible ENTRY BLOCK in front of such a
kernel -- s_load of the preloaded dwords off s[0:1], a wait, s_branch over an alignment gap -- which firmware that preloads skips; the
audit looks at the BODY behind it, and only at scalar loads, waits and the kernel descriptor.
usage: kernarg_audit.py file.s ...   (hipcc -S --cuda-device-only output of mq_quantize.hip / mq_gemm.hip, the build's flags)
  every quantize_tiled8_kernel<V, HAS_SUM, GRPS>
    PRELOAD  the descriptor's kernarg_preload_length covers the whole parameter list (the metadata's explicit arguments)
    KERNARG  no s_load_dword* off s[0:1] (the kernarg pointer, until the code reuses the pair) anywhere in the body
  gemm_i8_fr_kernel
    PRELOAD  the preload length covers the leading scalars: every parameter in front of the first struct passed by value
    WAIT     between the entry block and the first global_load* at most ONE s_waitcnt names lgkmcnt -- the trailing struct's, whose
             per-n pointers the program's first requests need (the grid pointers' own dereferences stand inside the program, behind
             those requests) -- and it stands late: every read of the struct is requested in front of it, and at least LATE
             instructions (the tile map: two integer divisions, ~100 scalar instructions) separate it from the body's first one
A violation prints `<file>:<line> PRELOAD|KERNARG|WAIT <kernel>: <what>`; the last line counts kernels and violations."""
import re
import sys

QUANTIZE = re.compile(r"^(_ZN2mq22quantize_tiled8_kernelILi(\d)ELb([01])ELi(\d)E\w*):")
GEMM = re.compile(r"^(_ZN2mq17gemm_i8_fr_kernelE\w*):")
KERNARG_LOAD = re.compile(r"^s_load_dword\w*\s+\S+\s+s\[0:1\]\s*,")
LATE = 32       # a wait in front of the tile map stands < 10 instructions into the body; one behind it > 100


def _instr(line):
    """the instruction text of a line, or '' for labels, directives, comments and blank lines"""
    t = line.split(";")[0].strip()
    return "" if (not t or t.endswith(":") or t.startswith(".")) else t


def _lgkm_wait(t):
    """an s_waitcnt that waits for scalar loads: it names lgkmcnt, or is a bare immediate (every counter)"""
    return t.startswith("s_waitcnt") and ("lgkmcnt" in t or re.match(r"^s_waitcnt\s+(0x[0-9a-f]+|\d+)$", t) is not None)


def _writes_kernarg_ptr(t):
    m = re.match(r"^s_\w+\s+(s\d+|s\[\d+:\d+\])\s*,", t)
    if not m or t.startswith(("s_cmp", "s_bitcmp", "s_waitcnt", "s_cbranch", "s_branch")):
        return False
    d = m.group(1)
    lo, hi = (int(d[1:]),) * 2 if "[" not in d else map(int, d[2:-1].split(":"))
    return lo <= 1 and hi >= 0


def body_start(lines, first, last):
    """the line behind the compiler's entry block (kernarg s_loads, waits, one s_branch), or `first` when the function has none"""
    for n in range(first + 1, last):
        t = _instr(lines[n])
        if not t:
            continue
        if t.startswith("s_branch"):
            return n + 1
        if not (KERNARG_LOAD.match(t) or t.startswith("s_waitcnt")):
            break
    return first + 1


def descriptor(lines, name):
    """{directive: int} of the kernel's .amdhsa_kernel block"""
    out = {}
    begin = next((n for n, l in enumerate(lines) if l.strip() == ".amdhsa_kernel " + name), None)
    if begin is None:
        return out
    for l in lines[begin + 1:]:
        if ".end_amdhsa_kernel" in l:
            break
        m = re.match(r"^\s*\.amdhsa_(\w+)\s+(-?\d+)\s*$", l)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def explicit_args(lines, name):
    """[(offset, size, value_kind)] of the kernel's explicit parameters, in order, from the code-object metadata"""
    at = next((n for n, l in enumerate(lines) if re.match(r"^\s+\.name:\s+%s\s*$" % re.escape(name), l)), None)
    if at is None:
        return []
    top = next((n for n in range(at, -1, -1) if lines[n].startswith("  - .")), 0)
    args, cur = [], None
    for l in lines[top:at]:
        if l.startswith("      - ."):
            cur = {}
            args.append(cur)
        elif not l.startswith("        ."):      # behind the argument list
            cur = None
        m = re.match(r"^\s+(?:- )?\.(offset|size|value_kind):\s+(\S+)", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return [(int(a["offset"]), int(a["size"]), a["value_kind"]) for a in args
            if {"offset", "size", "value_kind"} <= set(a) and not a["value_kind"].startswith("hidden_")]


def _preload(lines, name, first, need_bytes, what):
    d = descriptor(lines, name)
    have = d.get("user_sgpr_kernarg_preload_length", 0)
    if need_bytes is None:
        return [(first + 1, "PRELOAD", "no parameter list in the metadata")]
    if have * 4 < need_bytes:
        return [(first + 1, "PRELOAD", "kernarg_preload_length %d (%d bytes) does not cover %s: %d bytes" % (have, have * 4, what, need_bytes))]
    return []


def audit_quantize(name, lines, first, last):
    args = explicit_args(lines, name)
    bad = _preload(lines, name, first, max((o + s for o, s, _ in args), default=None), "the parameter list")
    for n in range(body_start(lines, first, last), last):
        t = _instr(lines[n])
        if KERNARG_LOAD.match(t):
            bad.append((n + 1, "KERNARG", "the body reads a kernel argument: %s" % t))
        if _writes_kernarg_ptr(t):
            break
    return bad


def audit_gemm(name, lines, first, last):
    args = explicit_args(lines, name)
    lead = []
    for o, s, kind in args:
        if kind == "by_value" and s > 8:
            break
        lead.append(o + s)
    bad = _preload(lines, name, first, max(lead, default=None), "the leading scalars")
    start = body_start(lines, first, last)
    body = [n for n in range(start, last) if _instr(lines[n])]
    load = next((n for n in body if _instr(lines[n]).startswith("global_load")), None)
    if load is None:
        return bad + [(first + 1, "WAIT", "no global_load in the function")]
    waits = [n for n in body if n < load and _lgkm_wait(_instr(lines[n]))]
    if len(waits) > 1:
        bad.append((waits[1] + 1, "WAIT", "%d scalar waits stand in front of the first vector request (line %d), want at most one" % (len(waits), load + 1)))
    if waits:
        w = waits[0]
        late = [n for n in body if w < n < load and KERNARG_LOAD.match(_instr(lines[n]))]
        if late:
            bad.append((late[0] + 1, "WAIT", "a kernel argument is requested behind the wait (line %d), in front of the first vector request" % (w + 1)))
        depth = len([n for n in body if n < w])
        if depth < LATE:
            bad.append((w + 1, "WAIT", "the scalar wait stands %d instructions into the body (want >= %d): in front of the tile map" % (depth, LATE)))
    return bad


def audit(path):
    """(number of kernels, [report lines]) of one assembly file"""
    lines = open(path).read().split("\n")
    out, count = [], 0
    for n, l in enumerate(lines):
        q, g = QUANTIZE.match(l), GEMM.match(l)
        if not (q or g):
            continue
        count += 1
        last = next((k for k in range(n, len(lines)) if lines[k].startswith(".Lfunc_end")), len(lines))
        if q:
            label = "quantize_tiled8_kernel<%d, %s, %d>" % (int(q.group(2)), "true" if q.group(3) == "1" else "false", int(q.group(4)))
            found = audit_quantize(q.group(1), lines, n, last)
        else:
            label, found = "gemm_i8_fr_kernel", audit_gemm(g.group(1), lines, n, last)
        for ln, kind, what in found:
            out.append("%s:%d %s %s: %s" % (path.split("/")[-1], ln, kind, label, what))
    return count, out


if __name__ == "__main__":
    for p in sys.argv[1:]:
        count, report = audit(p)
        for line in report:
            print(line)
        print(p.split("/")[-1], "audited kernels", count, "kernel-argument violations", len(report))
