"""What a node-group sweep kernel waits for between the last store of a node visit and the first MFMA of the next one, from the
compiler's ISA listing.

    python tools/isa_visit_waits.py [--flags "-DHG_VISIT_WAITS=0"] [--keep DIR] [--from DIR]

compiles pyfaceanalysis_amd/csrc/hg_fused.hip and hg_fused_sum.hip to assembly with the project's flags (--from DIR: reads
DIR/hg_fused.s and DIR/hg_fused_sum.s instead) and prints one line per kernel: layer 2's, layer 3's, k_stage_sum<4, 4, T, true>
for T = 2 and 1, and k_stage_sum_pair<1>.  Every path the code can take from a global_store to the first MFMA it reaches without
meeting another store or a barrier is a span (a branch is followed both ways, a block once per path; a forward branch over
MFMAs, the guard of a block's unused k-steps, is not taken).  A span is written as the instructions in
it: L for a global_load, wN for an s_waitcnt with vmcnt(N).  For each wait, k is the number of loads of the span issued before it
and s the stores of the visit just ended (the run of stores the span starts from, conditional ones included): the counter retires
in order, so the wait
    retires stores of that visit     when N < k + s   (the number it can retire: k + s - N, at most s),
    waits for a load of the span     when N < k       (a second-child load issued and awaited where the visit begins).
The line gives the spans (distinct ones, with the number of paths), the worst of both figures over all spans, the kernel's
registers and its scratch bytes."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyfaceanalysis_amd", "csrc")
KERNELS = [
    ("hg_fused", "k_stageILi3ELi3ELi2ELb0ELb1ELi3ELb1ELi1EE", "k_stage<3,3,2,false,true,3,true,1>"),
    ("hg_fused", "k_stageILi4ELi4ELi2ELb0ELb0ELi0ELb1ELin1EE", "k_stage<4,4,2,false,false,0,true,-1>"),
    ("hg_fused_sum", "k_stage_sumILi4ELi4ELi2ELb1EE", "k_stage_sum<4,4,2,true>"),
    ("hg_fused_sum", "k_stage_sumILi4ELi4ELi1ELb1EE", "k_stage_sum<4,4,1,true>"),
    ("hg_fused_sum", "k_stage_sum_pairILi1EE", "k_stage_sum_pair<1>"),
]
MAX_PATHS = 20000


def kernel_text(lines, key):
    a = next(i for i, l in enumerate(lines) if l.startswith("_Z") and key in l.split(":")[0] and l.split(":")[0].endswith("StageParamsE"))
    b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
    meta = {}
    for l in lines[b:b + 80]:
        m = re.match(r";\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy):\s*(\d+)", l)
        if m:
            meta.setdefault(m.group(1), int(m.group(2)))
    return lines[a + 1:b], meta


def parse(body):
    """-> instructions [(op, argument text)], label -> index of the instruction that follows it"""
    ins, labels = [], {}
    for l in body:
        s = l.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"(\.LBB\d+_\d+):", s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if s.startswith("."):
            continue
        p = s.split(None, 1)
        ins.append((p[0], p[1] if len(p) > 1 else ""))
    return ins, labels


def spans_from(ins, labels, start):
    """every path from the instruction after `start` to the first MFMA: the loads and vmcnt waits on it"""
    out, stack, n = [], [(start + 1, (), frozenset())], 0
    while stack and n < MAX_PATHS:
        i, seq, seen = stack.pop()
        while i < len(ins):
            op, arg = ins[i]
            if op.startswith("v_mfma"):
                out.append(seq)
                n += 1
                break
            if op.startswith("global_store") or op in ("s_endpgm", "s_barrier"):      # a barrier: the node group is over, not a next visit
                break
            if op.startswith("global_load"):
                seq += ("L",)
            elif op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", arg)
                if m:
                    seq += ("w" + m.group(1),)
            elif op == "s_branch" or op.startswith("s_cbranch"):
                t = labels[arg.strip()]
                if op != "s_branch":
                    if any(o.startswith("v_mfma") for o, _ in ins[i + 1:t]):      # a forward branch over MFMAs guards k-steps: not taken
                        i += 1
                        continue
                    stack.append((i + 1, seq, seen))
                if t in seen:
                    break
                seen = seen | {t}
                i = t
                continue
            i += 1
    return out


def stores_before(ins, at):
    """the run of stores that ends at `at`: back to the nearest MFMA"""
    s, i = 0, at
    while i >= 0 and not ins[i][0].startswith("v_mfma"):
        s += ins[i][0].startswith("global_store")
        i -= 1
    return s


def describe(ins, labels):
    spans, retired, own = {}, 0, 0
    for at, (op, _) in enumerate(ins):
        if not op.startswith("global_store"):
            continue
        s = stores_before(ins, at)
        for seq in spans_from(ins, labels, at):
            k, txt = 0, []
            for e in seq:
                if e == "L":
                    k += 1
                else:
                    n = int(e[1:])
                    retired = max(retired, min(s, max(0, k + s - n)))
                    own = max(own, max(0, k - n))
                txt.append(e)
            key = "%d stores, then %s" % (s, " ".join(txt) if txt else "nothing")
            spans[key] = spans.get(key, 0) + 1
    return spans, retired, own


def main():
    arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
    src_dir = arg("--from")
    d = src_dir or arg("--keep") or tempfile.mkdtemp()
    os.makedirs(d, exist_ok=True)
    if not src_dir:
        procs = [subprocess.Popen(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S"] + (arg("--flags") or "").split()
                                  + [os.path.join(CSRC, unit + ".hip"), "-o", os.path.join(d, unit + ".s")], stderr=subprocess.DEVNULL)
                 for unit in ("hg_fused", "hg_fused_sum")]
        if any(p.wait() for p in procs):
            sys.exit("hipcc failed")
    text = {unit: open(os.path.join(d, unit + ".s")).read().splitlines() for unit in ("hg_fused", "hg_fused_sum")}
    for unit, key, name in KERNELS:
        body, meta = kernel_text(text[unit], key)
        ins, labels = parse(body)
        spans, retired, own = describe(ins, labels)
        top = sorted(spans.items(), key=lambda kv: (-kv[1], kv[0]))
        what = "; ".join("%s (%d path%s)" % (k, n, "" if n == 1 else "s") for k, n in top[:6]) + (" (+%d other spans)" % (len(top) - 6) if len(top) > 6 else "")
        print("%s: %d VGPRs, %d AGPRs, %d B scratch, occupancy %d | a wait of a span retires up to %d stores of the visit just ended and waits for up to %d "
              "loads issued in the span | %s" % (name, meta.get("NumVgprs", -1), meta.get("NumAgprs", -1), meta.get("ScratchSize", -1), meta.get("Occupancy", -1),
                                                 retired, own, what))


if __name__ == "__main__":
    main()
