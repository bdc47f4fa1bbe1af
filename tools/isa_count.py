"""Static instruction counts of the small step kernel, one wave's path at a time.

Compiles wab_step_small.hip with -DWAB_ONLY_WAVE=k (the other waves' functions dead-code
eliminated; not a runnable build) and counts VALU / SALU / LDS / VMEM instructions of the
default-geometry kernel wab_step_small<8, 11, false, false, false>, plus the store-only remainder (k = 9).
Loops count once, so this ranks the straight-line cost of each wave's step, the part a
PMC run cannot split by wave.  Usage: python tools/isa_count.py [extra hipcc flags]

--roll-store [extra hipcc flags]: the rollout instance wab_step_small<8, 11, false, true, false>, waves
W0 and W2: static counts of each obs store region, from a region's first stream read
(ds_read_u16) to its last 16-byte global store.  A region is `general` (per-unit masked, the
partial-group path: it clears with ds_write_b16) or `whole` (store_units_whole11: ds_write_b128
clears); 11-12 stores = a step's store_units_nt, 5-6 = the last step's store_units_of.

--roll-loop [extra hipcc flags]: the default-rules rollout instance wab_step_small<8, 11, false,
true, true> (ISA_ROLL_KERNEL: another one, e.g. the generic ..ELb1ELb0EEE..), one wave at a time:
static counts of the wave's step loop, the outermost loop that holds the step's barriers.  Scalar
loads (the 64-byte load of the step's actions apart), SALU, branches, s_waitcnt and the full
lgkmcnt(0) ones among them, LDS instructions, v_readlane / v_writelane (scalars kept in VGPR
lanes).  Code on every path counts once, the first and last step's and the rare branches
included (where the default-rules instance loads the state pointers it needs there).
"""
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "wab_gym_amd", "csrc", "wab_step_small.hip")
KERNEL = os.environ.get("ISA_KERNEL", "_ZN3wab14wab_step_smallILi8ELi11ELb0ELb0ELb0EEEvNS_6ParamsE")


ROLL_KERNEL = "_ZN3wab14wab_step_smallILi8ELi11ELb0ELb1ELb0EEEvNS_6ParamsE"
ROLL_RULES_KERNEL = os.environ.get("ISA_ROLL_KERNEL", "_ZN3wab14wab_step_smallILi8ELi11ELb0ELb1ELb1EEEvNS_6ParamsE")


def listing(flags, kernel, out="/tmp/isa_count.s"):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DWAB_DIAGNOSTIC_BUILD",
                           "--cuda-device-only", "-S", SRC, "-o", out] + flags, stderr=subprocess.DEVNULL)
    s = open(out).read()
    a = s.index(kernel + ":")
    ops = []
    for line in s[a:s.index(".Lfunc_end", a)].splitlines():
        m = re.match(r"\s+([a-z_0-9]+)(.*)", line)
        if m:
            ops.append((m.group(1), m.group(2)))
    return ops


def store_regions(ops):
    """[first ds_read_u16 .. last global_store_dwordx4] spans: a new span starts at a stream
    read that follows a store (every path issues its reads before its first store)."""
    spans, start, last_store = [], None, None
    for i, (op, _) in enumerate(ops):
        if op == "ds_read_u16":
            if start is None or last_store is not None:
                if start is not None:
                    spans.append((start, last_store))
                start, last_store = i, None
        elif op in ("global_store_dwordx4", "flat_store_dwordx4") and start is not None:
            last_store = i
        elif op == "s_barrier" and start is not None:
            if last_store is not None:
                spans.append((start, last_store))
            start, last_store = None, None
    if start is not None and last_store is not None:
        spans.append((start, last_store))
    rows = []
    for a, b in spans:
        c = {"kind": "general", "stores": 0, "valu": 0, "salu": 0, "branch": 0, "exec_branch": 0, "waitcnt": 0, "lds": 0}
        for op, rest in ops[a:b + 1]:
            if op.startswith("v_"):
                c["valu"] += 1
            elif op.startswith("ds_"):
                c["lds"] += 1
                if op == "ds_write_b128":
                    c["kind"] = "whole"
            elif op.endswith("store_dwordx4"):
                c["stores"] += 1
            elif op.startswith("s_cbranch"):
                c["branch"] += 1
                c["exec_branch"] += op.startswith("s_cbranch_exec")
            elif op == "s_waitcnt":
                c["waitcnt"] += 1
            elif op.startswith("s_") and op not in ("s_nop", "s_barrier"):
                c["salu"] += 1
        rows.append(c)
    return rows


def step_loop(path, kernel):
    """The instructions of the kernel's step loop: the outermost loop (a label and a later
    branch back to it) with an s_barrier inside, the largest one if there are several, with the
    blocks of it that are laid out behind its back edge."""
    s = open(path).read()
    a = s.index("\n" + kernel + ":")
    labels, ins = {}, []
    for line in s[a:s.index(".Lfunc_end", a)].splitlines():
        m = re.match(r"(\.LBB[0-9_]+):", line)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        m = re.match(r"\s+([a-z_0-9]+)\s*(.*)", line)
        if m and not line.lstrip().startswith((".", ";")):
            ins.append((m.group(1), m.group(2)))
    loops = []
    for i, (op, rest) in enumerate(ins):
        if (op.startswith("s_cbranch") or op == "s_branch") and labels.get(rest.split()[0], i + 1) <= i:
            a0 = labels[rest.split()[0]]
            loops.append((a0, i))
    steps = [l for l in loops if any(o == "s_barrier" for o, _ in ins[l[0]:l[1] + 1])]
    if not steps:
        return []
    a0, b0 = max(steps, key=lambda l: l[1] - l[0])
    # blocks of the loop laid out after its first back edge end in a branch back into it
    grown = True
    while grown:
        grown = False
        for a1, b1 in loops:
            if a0 <= a1 <= b0 < b1 or a1 < a0 <= b1 <= b0:
                a0, b0, grown = min(a0, a1), max(b0, b1), True
    return ins[a0:b0 + 1]


def loop_counts(ops):
    c = {"instr": len(ops), "s_load": 0, "actions_x16": 0, "salu": 0, "branch": 0, "waitcnt": 0, "lgkmcnt0": 0,
         "lds": 0, "lane": 0, "valu": 0, "vmem": 0}
    for op, rest in ops:
        if op.startswith("s_load") or op.startswith("s_buffer_load"):
            if op.endswith("x16"):
                c["actions_x16"] += 1
            else:
                c["s_load"] += 1
        elif op.startswith("s_cbranch") or op == "s_branch":
            c["branch"] += 1
        elif op == "s_waitcnt":
            c["waitcnt"] += 1
            c["lgkmcnt0"] += "lgkmcnt(0)" in rest
        elif op in ("v_readlane_b32", "v_writelane_b32"):
            c["lane"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("s_") and op not in ("s_nop", "s_barrier", "s_setprio"):
            c["salu"] += 1
    return c


def roll_loop(extra):
    from concurrent.futures import ThreadPoolExecutor

    def one(k):
        out = "/tmp/isa_count_w%d.s" % k
        listing(["-DWAB_ONLY_WAVE=%d" % k] + extra, ROLL_RULES_KERNEL, out)
        return loop_counts(step_loop(out, ROLL_RULES_KERNEL))

    with ThreadPoolExecutor(4) as ex:
        rows = list(ex.map(one, range(4)))
    keys = list(rows[0])
    print("%-12s" % "wave" + "".join("%12s" % k for k in keys))
    for k, name in enumerate(("W0 bushes", "W1 draws", "W2 wolves", "W3 ring")):
        print("%-12s" % name + "".join("%12d" % rows[k][key] for key in keys))


def counts(flags):
    out = "/tmp/isa_count.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DWAB_DIAGNOSTIC_BUILD",
                           "--cuda-device-only", "-S", SRC, "-o", out] + flags, stderr=subprocess.DEVNULL)
    s = open(out).read()
    a = s.index(KERNEL + ":")
    body = s[a:s.index(".Lfunc_end", a)].splitlines()
    c = {"valu": 0, "salu": 0, "lds": 0, "vmem": 0}
    for line in body:
        m = re.match(r"\s+([a-z_0-9]+)", line)
        if not m:
            continue
        op = m.group(1)
        if op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_")):
            c["vmem"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    return c


if __name__ == "__main__":
    extra = sys.argv[1:]
    if extra and extra[0] == "--roll-loop":
        roll_loop(extra[1:])
        sys.exit(0)
    if extra and extra[0] == "--roll-store":
        for k in (0, 2):
            for c in store_regions(listing(["-DWAB_ONLY_WAVE=%d" % k] + extra[1:], ROLL_KERNEL)):
                print("W%d %s" % (k, c))
        sys.exit(0)
    for k, name in ((0, "W0 bushes"), (1, "W1 draws"), (2, "W2 wolves"), (3, "W3 ring"), (9, "stores only")):
        print("%-12s %s" % (name, counts(["-DWAB_ONLY_WAVE=%d" % k] + extra)))
