"""What the fused executor launches, call by call: one ``execute_device`` per batch size on nets that between them take every route of
the call plan (csrc/hg_fused_call.hpp) — the synthetic U11L-128, U11L-64 and the 96-pixel linear U11L, ``prod_uneven``, ``ig_c``,
``igfold2`` and ``mixed`` of tests/stage_shape_cases.py and tests/pair_cases.three_pair_net under the switches that store its links
summed — at 1, 17, 70, 130, 340, 425, 728, 1024, 1738 and 4096 rows.  Every handle is planned under HIGSFA_DEBUG, so stderr carries
one line per launch.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/launch_sequence.py 2> DIR/debug.txt
    HIGSFA_LIB=tools/ab/libhigsfa_<tag>.so rocprofv3 ... (the same, with another build of the library: tools/build_ref_lib.sh)
    python tools/launch_sequence.py --compare DIR_A DIR_B

--compare reads the two kernel traces and the two debug texts (no GPU): the traces must agree launch for launch in kernel name, grid,
workgroup and LDS size, and the debug lines both libraries know ("[front]", "[igsfa stage", "[prod stage", "[pair stage") must be the
same text.  A fresh process per run, each under its own time limit; never together with counters."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = (1, 17, 70, 130, 340, 425, 728, 1024, 1738, 4096)
SWEEP_ONLY_PAIRED = {"HIGSFA_SPLITM_MAX": "0", "HIGSFA_SPLITM_WGS": "0", "HIGSFA_TAIL": "0", "HIGSFA_SUBTREE": "0", "HIGSFA_SUM_LDS": "128", "HIGSFA_PAIR_WGS": "1"}
OLD_LINES = ("[front]", "[igsfa stage", "[prod stage", "[pair stage")


def nets():
    """[(name, nodes or blob, switches)]"""
    from pyfaceanalysis_amd import synth
    from tests import helpers, pair_cases
    from tests import stage_shape_cases as cases
    out = [(n, synth.cached_preset_blob(n)[0], {}) for n in ("U11L-128", "U11L-64")]
    out.append(("U11L-96", helpers.linear_u11l_96(), {}))
    shape_nets = cases.nets()
    out += [(n, shape_nets[n][0](), shape_nets[n][1]) for n in ("prod_uneven", "ig_c", "igfold2", "mixed")]
    out.append(("three_pair", pair_cases.three_pair_net(), SWEEP_ONLY_PAIRED))
    return out


def run():
    import numpy as np
    import torch
    from pyfaceanalysis_amd.flow import Flow
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name, net, env in nets():
        for k, v in dict(env, HIGSFA_DEBUG="1").items():
            os.environ[k] = v
        flow = Flow.from_blob(net, device=0, output_dtype=np.float32) if isinstance(net, bytes) else Flow(net, output_dtype=np.float32)
        info = flow.info()      # plans the handle under the switches
        for k in dict(env, HIGSFA_DEBUG="1"):
            del os.environ[k]
        d_in, d_out = flow.input_dim, flow.output_dim
        x = torch.from_numpy(np.random.default_rng(1).normal(size=(ROWS[-1], d_in)).astype(np.float32)).to(dev)
        y = torch.empty((ROWS[-1], d_out), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        for n in ROWS:
            sys.stderr.write("== %s plan %d rows %d\n" % (name, info.plan_kind, n))
            sys.stderr.flush()
            flow.execute_device(x.data_ptr(), np.dtype(np.float32), n, d_in, y.data_ptr(), np.float32, d_out, d_out, stream=stream)
            torch.cuda.synchronize(dev)
            flow.check_errors()
        flow.close()
    print("launch_sequence: %d nets x %d batch sizes" % (len(nets()), len(ROWS)))


def trace_rows(folder):
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("%s: %d kernel traces" % (folder, len(files)))
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    keys = [k for k in rows[0] if k.startswith(("Grid_Size", "Workgroup_Size", "LDS_Block_Size"))]
    assert len(keys) >= 7, list(rows[0])
    return [(r["Kernel_Name"],) + tuple(int(r[k]) for k in keys) for r in rows]


def compare(a, b):
    ta, tb = trace_rows(a), trace_rows(b)
    diff = [i for i, (p, q) in enumerate(zip(ta, tb)) if p != q]
    print("kernel traces: %d | %d launches, %d differ (name, grid, workgroup, LDS)" % (len(ta), len(tb), len(diff) + abs(len(ta) - len(tb))))
    for i in diff[:5]:
        print("  launch %d:\n    %s\n    %s" % (i, ta[i], tb[i]))
    own = sum(1 for r in ta if "hg" in r[0])
    print("  of them the library's own kernels: %d, in %d distinct (name, grid, workgroup, LDS)" % (own, len({r for r in ta if "hg" in r[0]})))

    def old_lines(folder):
        with open(os.path.join(folder, "debug.txt")) as f:
            return [ln for ln in f.read().splitlines() if ln.startswith(OLD_LINES) or ln.startswith("== ")]
    la, lb = old_lines(a), old_lines(b)
    print("debug lines both libraries write: %d | %d, %s" % (len(la), len(lb), "identical text" if la == lb else "DIFFERENT"))
    ok = not diff and len(ta) == len(tb) and la == lb
    print("verdict: %s" % ("same launches" if ok else "the launches differ"))
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        raise SystemExit(compare(sys.argv[2], sys.argv[3]))
    run()
