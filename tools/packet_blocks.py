#!/usr/bin/env python3
"""Static instruction counts of the packet walk's loop in one gfx950 kernel, per basic block.

Cross-compiles pysicalbasedraytracer_amd/csrc/pbr_kernels.hip to assembly with the Makefile's flags
(device only, no GPU needed) — or reads an assembly file made that way (--asm) — finds the kernel
whose demangled name contains KERNEL, and prints one row per basic block of each packet loop: the
innermost loop (by the compiler's own loop comments) around a block that fetches a quad node's rows
through the scalar cache (at least five s_load_dwordx4/x8).  Instructions are counted by unit prefix:

  valu    v_*                       salu    s_* other than the ones below
  smem    s_load_* / s_buffer_load_*   lds   ds_*
  vmem    global_* flat_* buffer_* scratch_*
  branch  s_branch / s_cbranch_*    wait    s_waitcnt / s_nop / s_barrier

The counts are static: what a block holds, not how often it runs.

    python tools/packet_blocks.py 'k_wf_shade<false, 5, false, 5, true, true, false>' 'k_wf_camera_extend<6, false>'
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pysicalbasedraytracer_amd", "csrc")
COLS = ["valu", "salu", "smem", "lds", "vmem", "branch", "wait"]


def make_var(name, extra=""):
    """A variable of the csrc Makefile as make expands it."""
    out = subprocess.run(["make", "-C", CSRC, "-pn", f"EXTRA={extra}"], capture_output=True, text=True).stdout
    vals = dict(re.findall(r"^(\w+) :?= (.*)$", out, re.M))

    def expand(s, depth=0):
        return re.sub(r"\$\((\w+)\)", lambda m: expand(vals.get(m.group(1), ""), depth + 1) if depth < 8 else "", s)
    return expand(vals[name])


def compile_asm(path, extra=""):
    hipcc = make_var("HIPCC", extra)
    flags = [f for f in make_var("FLAGS", extra).split() if f]
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", "-o", path, "pbr_kernels.hip"]
    print("# " + " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, cwd=CSRC, check=True, stderr=subprocess.DEVNULL)


def demangle(names):
    filt = os.path.join(os.path.dirname(os.path.realpath(make_var("HIPCC"))), "..", "lib", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = "c++filt"
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def unit(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith(("s_load_", "s_buffer_load_")):
        return "smem"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_endpgm")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return None


class Block:
    def __init__(self, label):
        self.label = label
        self.n = collections.Counter()
        self.wide = 0        # s_load_dwordx4 / x8
        self.header = False  # a loop header
        self.inner = None    # innermost loop's header label (itself for a header)
        self.parents = []    # a header's enclosing loop headers


def kernel_blocks(lines, start):
    """The basic blocks of the function whose label is at lines[start]."""
    blocks = [Block("entry")]
    i = start + 1
    while i < len(lines):
        s = lines[i]
        if s.startswith(".Lfunc_end"):
            break
        # a block starts at a label, or at the comment the compiler leaves where a block is only fallen into
        m = re.match(r"(\.LBB\d+_\d+):\s*(;.*)?$", s) or re.match(r"; %bb\.(\d+):\s*(;.*)?$", s)
        if m:
            b = Block(m.group(1) if m.group(1).startswith(".") else ".Lbb." + m.group(1))
            c = m.group(2) or ""
            while i + 1 < len(lines) and re.match(r"\s+;", lines[i + 1]):   # the loop comment's further lines
                i += 1
                c += "\n" + lines[i]
            if "Loop Header" in c:
                b.header, b.inner = True, b.label[2:]
                b.parents = re.findall(r"Parent Loop (BB\d+_\d+)", c)   # outermost first
            else:
                h = re.search(r"in Loop: Header=(BB\d+_\d+)", c)
                b.inner = h.group(1) if h else None
            blocks.append(b)
        else:
            t = s.split(";")[0].split()
            if t and not t[0].startswith(".") and not t[0].endswith(":"):
                u = unit(t[0])
                if u:
                    blocks[-1].n[u] += 1
                if re.match(r"s_load_dwordx(4|8)$", t[0]):
                    blocks[-1].wide += 1
        i += 1
    return blocks


def loops_of(blocks):
    """label of a block → the headers of every loop around it, innermost first."""
    parents = {b.label[2:]: b.parents for b in blocks if b.header}
    out = {}
    for b in blocks:
        if b.inner is None:
            out[b.label] = []
        elif b.header:
            out[b.label] = [b.inner] + list(reversed(b.parents))
        else:
            out[b.label] = [b.inner] + list(reversed(parents.get(b.inner, [])))
    return out


def report(name, blocks, out):
    around = loops_of(blocks)
    fetch = [b for b in blocks if b.wide >= 5 and around[b.label]]
    total = collections.Counter()
    for b in blocks:
        total.update(b.n)
    print(f"### `{name}`\n", file=out)
    print("whole kernel: " + ", ".join(f"{c} {total[c]}" for c in COLS) + "\n", file=out)
    seen = []
    for f in fetch:
        loop = around[f.label][0]
        if loop in seen:
            continue
        seen.append(loop)
        body = [b for b in blocks if loop in around[b.label]]
        print(f"packet loop {len(seen)} (header {loop}, {len(body)} blocks)\n", file=out)
        print("| block | " + " | ".join(COLS) + " | note |", file=out)
        print("|---|" + "---:|" * len(COLS) + "---|", file=out)
        s = collections.Counter()
        for b in body:
            s.update(b.n)
            depth = len(around[b.label]) - len(around[".L" + loop])
            note = ("node fetch" if b.wide >= 5 else "") + (f" inner loop +{depth}" if depth > 0 else "")
            print(f"| {b.label[2:]} | " + " | ".join(str(b.n[c]) for c in COLS) + f" | {note.strip()} |", file=out)
        print("| **loop** | " + " | ".join(f"**{s[c]}**" for c in COLS) + " | |\n", file=out)
    if not fetch:
        print("(no block of a loop fetches a quad node's rows through the scalar cache)\n", file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernels", nargs="+", help="substrings of demangled kernel names (the first match is taken)")
    ap.add_argument("--asm", help="an assembly file already made with the Makefile's flags and --cuda-device-only -S")
    ap.add_argument("--extra", default="", help="the Makefile's EXTRA (additional compiler flags)")
    a = ap.parse_args()
    path = a.asm
    tmp = None
    if path is None:
        tmp = tempfile.mkdtemp()
        path = os.path.join(tmp, "pbr_kernels.s")
        compile_asm(path, a.extra)
    with open(path) as f:
        lines = f.read().splitlines()
    starts = {m.group(1): i for i, s in enumerate(lines) for m in [re.match(r"(_Z\w+):", s)] if m}
    names = demangle(list(starts))
    rc = 0
    for k in a.kernels:
        hit = [mn for mn, dn in names.items() if k in dn]
        if not hit:
            print(f"no kernel matches {k!r}", file=sys.stderr)
            rc = 1
            continue
        report(names[hit[0]], kernel_blocks(lines, starts[hit[0]]), sys.stdout)
    if tmp:
        os.remove(path)
        os.rmdir(tmp)
    return rc


if __name__ == "__main__":
    sys.exit(main())
