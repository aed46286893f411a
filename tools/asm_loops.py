"""Static instruction counts of the loops of a kernel, from the assembly hipcc -S leaves (gfx950): for every function the straight
instructions and, per loop (a backward branch to a label), the instructions and the v_mad_u64_u32 of its body, nested loops listed
with their parent. The rolled loops of poseidon.h (`#pragma unroll 1`) come out one to one, so a body times its trip count is the
dynamic count of that part of a permutation (profiles/poseidon_recurrence_resource_usage.txt).
python tools/asm_loops.py file.s [substring of the kernel names to list]"""
import re
import subprocess
import sys


def functions(path):
    """{name: [(label or None, mnemonic or None, branch target or None)]} per function of the file"""
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not line.startswith(".L"):
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            cur.append((m.group(1), None, None))
            continue
        m = re.match(r"^\t([a-z][\w]*)\b(.*)$", line)
        if m and not line.startswith("\t."):
            t = re.search(r"(\.LBB\d+_\d+)", m.group(2)) if m.group(1).startswith("s_cbranch") or m.group(1) == "s_branch" else None
            cur.append((None, m.group(1), t.group(1) if t else None))
    return out


def loops(items):
    """[(first, last, instructions, mads, depth)] of the backward branches, outermost first"""
    pos, n, idx = {}, 0, []
    for lab, ins, tgt in items:
        if lab:
            pos[lab] = n
        else:
            idx.append((n, ins, tgt))
            n += 1
    found = sorted({(pos[tgt], i) for i, ins, tgt in idx if tgt in pos and pos[tgt] <= i})
    mad = [1 if ins == "v_mad_u64_u32" else 0 for _, ins, _ in idx]
    res = []
    for a, b in found:
        depth = sum(1 for c, d in found if c <= a and b <= d and (c, d) != (a, b))
        res.append((a, b, b - a + 1, sum(mad[a:b + 1]), depth))
    return n, sum(mad), res


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True, timeout=20).stdout.strip() or name
    except (OSError, subprocess.TimeoutExpired):
        return name


if __name__ == "__main__":
    want = sys.argv[2] if len(sys.argv) > 2 else ""
    for name, items in functions(sys.argv[1]).items():
        d = re.sub(r"\(.*\)$", "", demangle(name)).replace("void ", "")
        if want not in d:
            continue
        n, mads, ls = loops(items)
        if not n:
            continue
        print("%s: %d instructions, %d v_mad_u64_u32" % (d, n, mads))
        for a, b, size, m, depth in ls:
            print("  %sloop at %6d..%6d: %6d instructions, %5d v_mad_u64_u32" % ("  " * depth, a, b, size, m))
