#!/usr/bin/env python3
"""Instruction mix of one kernel's main loop, by opcode class and by source region (static, from `hipcc -S -gline-tables-only`).

    python tools/isa_profile.py bl_shade_fast.hip fused_kernelILb1 [--lines] [--whole] [--flags "-DX ..."]

The main loop is the longest span between a label and a backward branch to it. Every instruction is attributed to the
source line of its `.loc` (innermost inlined frame) and grouped by the function that line belongs to (ctags-free: the
nearest preceding line that looks like a function header in that file). This is how round 3's judge found the v_mov /
v_readlane share of bl_shade_fused_kernel; profiles/r04_isa_mix_*.txt are its outputs.
"""
import collections
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "blacklight_amd", "csrc")


def classify(op):
    if op.startswith("v_"):
        if op.startswith(("v_mov_b32", "v_mov_b64", "v_accvgpr")):
            return "v_mov"
        if op.startswith(("v_readlane", "v_readfirstlane")):
            return "v_readlane"
        if op.startswith("v_writelane"):
            return "v_writelane"
        if op.startswith("v_cndmask"):
            return "v_cndmask"
        if op.startswith("v_cvt"):
            return "v_cvt"
        if op.startswith("v_cmp"):
            return "v_cmp"
        if "f64" in op:
            return "v_f64"
        return "v_other"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith(("s_load", "s_buffer_load")):
        return "s_load"
    if op.startswith(("s_cbranch", "s_branch")):
        return "s_branch"
    if op.startswith("s_"):
        return "salu"
    return "other"


FUNC_HEADER = re.compile(r"^\s*(?:template\s*<[^>]*>\s*)?(?:static\s+|inline\s+|constexpr\s+|__device__\s+|__host__\s+|__forceinline__\s+|__global__\s+|BLM_FN\s+|BLM_INLINE\s+)+[\w:<>\*&\s]+?\b(\w+)\s*\(")


def function_of(path, line, cache={}):
    if path not in cache:
        heads = []
        try:
            for n, text in enumerate(open(path, errors="replace"), 1):
                m = FUNC_HEADER.match(text)
                if m and not text.strip().startswith(("return", "if", "for", "while")):
                    heads.append((n, m.group(1)))
        except OSError:
            pass
        cache[path] = heads
    name = "?"
    for n, f in cache[path]:
        if n <= line:
            name = f
        else:
            break
    return name


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    by_line = "--lines" in sys.argv
    whole = "--whole" in sys.argv
    extra = []
    if "--flags" in sys.argv:
        extra = sys.argv[sys.argv.index("--flags") + 1].split()
        args = [a for a in args if a != sys.argv[sys.argv.index("--flags") + 1]]
    src, pattern = args[0], args[1]
    out = f"/tmp/bl_isa_{os.path.basename(src)}_{os.getpid()}.s"
    subprocess.run(["hipcc", "-S", "--offload-device-only", "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-mllvm",
                    "-disable-machine-licm", "-gline-tables-only", f"-I{REPO}/include", f"-I{CSRC}", os.path.join(CSRC, src), "-o", out] + extra,
                   check=True, capture_output=True)
    files = {}
    body = []   # (label or None, op, file, line)
    inside = False
    cur = (None, 0)
    for text in open(out):
        m = re.match(r"^\s*\.file\s+(\d+)\s+\"([^\"]*)\"(?:\s+\"([^\"]*)\")?", text)
        if m:
            files[int(m.group(1))] = os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
            continue
        m = re.match(r"^(_Z\w+):", text)
        if m:
            inside = pattern in m.group(1)
            if inside:
                kernel = m.group(1)
            continue
        if not inside:
            continue
        if text.startswith(".Lfunc_end"):
            inside = False
            continue
        m = re.match(r"^\s*\.loc\s+(\d+)\s+(\d+)", text)
        if m:
            cur = (int(m.group(1)), int(m.group(2)))
            continue
        m = re.match(r"^(\.LBB\w+):", text)
        if m:
            body.append((m.group(1), None, None, 0))
            continue
        if not text.startswith("\t"):
            continue
        op = text.strip().split()[0] if text.strip() else ""
        if not op or op.startswith((".", ";")):
            continue
        target = None
        if op.startswith(("s_cbranch", "s_branch")):
            target = text.strip().split()[1]
        body.append((None, op, files.get(cur[0], "?"), cur[1], target))
    # main loop: longest label .. backward branch span
    label_at = {b[0]: i for i, b in enumerate(body) if b[0]}
    best = (0, 0, len(body))
    for i, b in enumerate(body):
        if b[0] is None and len(b) > 4 and b[4] in label_at and label_at[b[4]] < i:
            span = i - label_at[b[4]]
            if span > best[0]:
                best = (span, label_at[b[4]], i + 1)
    lo, hi = (0, len(body)) if whole else (best[1], best[2])
    insts = [b for b in body[lo:hi] if b[0] is None]
    print(f"{kernel}: {'whole kernel' if whole else 'main loop'} {len(insts)} instructions")
    classes = collections.Counter(classify(b[1]) for b in insts)
    valu = sum(v for k, v in classes.items() if k.startswith("v_") and k not in ())
    print(f"  VALU {valu}: " + ", ".join(f"{k} {classes[k]}" for k in ("v_f64", "v_mov", "v_readlane", "v_writelane", "v_cndmask", "v_cvt", "v_cmp", "v_other")))
    print("  other: " + ", ".join(f"{k} {classes[k]}" for k in ("salu", "s_load", "s_waitcnt", "s_branch", "lds", "vmem", "other")))
    groups = collections.defaultdict(collections.Counter)
    for b in insts:
        path = b[2]
        key = f"{os.path.basename(path)}:{b[3]}" if by_line else f"{os.path.basename(path)}:{function_of(path, b[3])}"
        groups[key][classify(b[1])] += 1
    rows = sorted(groups.items(), key=lambda kv: -sum(kv[1].values()))
    print(f"  {'region':58s} {'all':>5s} {'f64':>5s} {'mov':>5s} {'lane':>5s} {'cnd':>5s} {'cvt':>5s} {'cmp':>5s} {'v_oth':>5s} {'salu':>5s} {'lds':>4s} {'vmem':>4s}")
    for key, c in rows[: (80 if by_line else 40)]:
        print(f"  {key[:58]:58s} {sum(c.values()):5d} {c['v_f64']:5d} {c['v_mov']:5d} {c['v_readlane'] + c['v_writelane']:5d} {c['v_cndmask']:5d} "
              f"{c['v_cvt']:5d} {c['v_cmp']:5d} {c['v_other']:5d} {c['salu'] + c['s_load'] + c['s_waitcnt'] + c['s_branch']:5d} {c['lds']:4d} {c['vmem']:4d}")


if __name__ == "__main__":
    main()
