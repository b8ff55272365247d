"""Inputs of the fused-plan digest test (tests/test_fused_plan_host.py) and of its sanitizer case (tests/test_sanitizers.py): the
flows whose plans are recorded in tests/golden/fused_plan_digests.json, and the stand-alone driver that prints a plan.

No linear-algebra result may reach a digest: the recorded file is compared on every machine, and what numpy computes through
BLAS / LAPACK (a matrix product such as SFANode's ``avg @ sf``, ``eigh`` in the presets' training) differs in its last bits from
one library or CPU to the next.  So every floating-point array of every flow here is drawn element by element from one seeded
numpy Generator (``reseed``) after the flow's structure is built; the presets are built as structures only, never trained."""
import functools
import json
import os
import subprocess

import numpy as np

from pyfaceanalysis_amd import blob, synth
from pyfaceanalysis_amd import nodes as N
from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyfaceanalysis_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_plan_digests.json")


def load_golden():
    """{case name: [recorded lines]}.  The file keeps every distinct line once ("lines") and each case as indices into them: the
    plans of one net under different switches share most of their stages."""
    with open(GOLDEN) as f:
        g = json.load(f)
    return {name: [g["lines"][i] for i in idx] for name, idx in g["cases"].items()}


def reseed(flow, seed):
    """Overwrite every weight array of the flow, in place, with draws from default_rng(seed); returns the flow."""
    rng = np.random.default_rng(seed)

    def visit(n):
        if isinstance(n, N.PCANode):
            n.avg = rng.normal(size=n.avg.shape)
            n.v = rng.normal(size=n.v.shape) / np.sqrt(n.input_dim)
        elif isinstance(n, N.SFANode):
            n.avg = rng.normal(size=n.avg.shape) * 0.1
            n.sf = rng.normal(size=n.sf.shape) / np.sqrt(n.input_dim)
            n._bias = rng.normal(size=n._bias.shape) * 0.1          # (MDP's avg @ sf: a BLAS result, replaced like the rest)
        elif isinstance(n, N.LinearRegressionNode):
            n.beta = rng.normal(size=n.beta.shape) / np.sqrt(n.beta.shape[0])
        elif isinstance(n, N.iGSFANode):
            n.x_mean = rng.normal(size=n.x_mean.shape)
            k = n.sfa_node.output_dim
            if n.scaling == "matrix":      # triangular with a positive diagonal: the loader can invert it
                n.scaling_matrix = np.triu(rng.normal(size=(k, k)) * 0.3, 1) + np.diag(rng.uniform(0.5, 2.0, size=k))
            else:
                n.magn_n_sfa_x = rng.uniform(0.5, 2.0, size=(1, k))
            for c in (n.sfa_node, n.lr_node, n.pca_node):
                if c is not None:
                    visit(c)
        elif isinstance(n, N.CloneLayer):
            visit(n.node)
        elif isinstance(n, N.Layer):
            for c in n.nodes:
                visit(c)
        elif isinstance(n, N.FlowNode):
            for c in n.flow:
                visit(c)

    for n in flow:
        visit(n)
    return flow


def preset_structure(name, node_kind="pca_exp_sfa"):
    """The nodes synth.build_preset(name, node_kind=...) returns, with zero weights and without training: the same switchboards,
    node classes and dimensions (synth.train_hierarchy's rules; test_preset_structures_are_the_presets compares them)."""
    side, f0, dims = synth.PRESETS[name]
    funcs = [N.identity, N.unsigned_08expo]
    flow, grid, ch = [], None, 1
    z = np.zeros
    for li, (p, s) in enumerate(dims):
        if li == 0:
            sb = N.Rectangular2dSwitchboard((side, side), (f0, f0), (f0, f0), 1)
        else:
            nx, ny = grid
            merge_x = (li % 2 == 1)
            if merge_x and nx == 1:
                merge_x = False
            if not merge_x and ny == 1:
                merge_x = True
            field = (2, 1) if merge_x else (1, 2)
            sb = N.Rectangular2dSwitchboard((nx, ny), field, field, ch)
        grid = sb.out_channels_xy
        n_nodes, d_in = sb.output_channels, sb.out_channel_dim
        if node_kind == "pca_exp_sfa":
            p_ = min(p, d_in)
            out_dim = min(s, 2 * p_)
            layer = N.Layer([N.FlowNode([N.WhiteningNode(z(d_in), z((d_in, p_))), N.GeneralExpansionNode(funcs, p_), N.SFANode(z(2 * p_), z((2 * p_, out_dim)))])
                             for _ in range(n_nodes)])
        else:
            out_dim = min(s, d_in)
            k = max(1, min(out_dim - 1, out_dim // 2)) if out_dim > 1 else 1
            layer = N.Layer([N.iGSFANode(z(d_in), N.GeneralExpansionNode(funcs, d_in), N.SFANode(z(2 * d_in), z((2 * d_in, k))), np.ones(k),
                                         N.LinearRegressionNode(z((k + 1, d_in))), N.PCANode(z(d_in), z((d_in, out_dim - k))), k) for _ in range(n_nodes)])
        flow += [sb, layer]
        ch = out_dim
        if n_nodes == 1 and li < len(dims) - 1:
            break
    return flow


def shape_of(n):
    """Class and dimensions of a node and everything below it (what a structure is, weights aside)."""
    kids = n.nodes if isinstance(n, N.Layer) else n.flow if isinstance(n, N.FlowNode) else \
        [c for c in (n.exp_node, n.sfa_node, n.lr_node, n.pca_node) if c is not None] if isinstance(n, N.iGSFANode) else []
    extra = tuple(n.connections.tolist()) if isinstance(n, N.Switchboard) else ()
    return (type(n).__name__, n.input_dim, n.output_dim, extra, tuple(shape_of(c) for c in kids))


@functools.lru_cache(maxsize=None)
def cases():
    """[(case name, {HIGSFA_* switch: value}, blob bytes)]: every planner branch at least once (the coverage test says which)."""
    flows = [("overlapping_net", helpers.overlapping_net()), ("linear_net", helpers.linear_net()), ("linear_u11l_96", helpers.linear_u11l_96()),
             ("product_net", helpers.product_net()), ("product_hier_net", helpers.product_hier_net()), ("wide_merge_net", helpers.wide_merge_net()),
             ("fuzz_product_net_3", helpers.fuzz_product_net(3)), ("remainder_net", helpers.remainder_net())]
    flows += [("fuzz_net_%d" % s, helpers.fuzz_net(s)) for s in (1, 3, 4)]
    flows += [("subtree_fuzz_net_%d" % s, helpers.subtree_fuzz_net(s)) for s in (0, 2)]
    flows += [(n, preset_structure(n)) for n in ("T3L-8", "T5L-16", "U11L-64", "U11L-128")]
    flows += [("U11L-128_igsfa", preset_structure("U11L-128", "igsfa"))]
    blobs = {name: blob.flow_to_blob(reseed(f, 100 + i)) for i, (name, f) in enumerate(flows)}
    out = [(name, {}, blobs[name]) for name, _ in flows]
    for s in (0, 1, 2, 10):
        b = blob.flow_to_blob(reseed(helpers.fuzz_igsfa_net(s), 200 + s))
        out += [("fuzz_igsfa_net_%d" % s, {}, b), ("fuzz_igsfa_net_%d+HIGSFA_IG_NOFOLD" % s, {"HIGSFA_IG_NOFOLD": "1"}, b)]
    for k, v in (("HIGSFA_NO_REM4", "1"), ("HIGSFA_NO_PACK", "1"), ("HIGSFA_NO_SOA", "1"), ("HIGSFA_TAIL", "0"), ("HIGSFA_SUBTREE", "0")):
        out.append(("U11L-128+%s=%s" % (k, v), {k: v}, blobs["U11L-128"]))
    return tuple(out)


SWITCHES = ("HIGSFA_NO_REM4", "HIGSFA_IG_NOFOLD", "HIGSFA_NO_PACK", "HIGSFA_NO_SOA", "HIGSFA_TAIL", "HIGSFA_SUBTREE", "HIGSFA_SUBTREE_WGS")


def build_driver(exe, extra_flags=()):
    """tests/plan_digest_driver.cpp with plain g++ against hg_tree.cpp and hg_fused_plan.cpp ONLY, no HIP library: if it does not
    link, a device buffer or a HIP call is back in the plan.  Returns the finished subprocess."""
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + list(extra_flags) + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "plan_digest_driver.cpp"), os.path.join(CSRC, "hg_tree.cpp"),
           os.path.join(CSRC, "hg_fused_plan.cpp"), "-o", str(exe)]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def run_driver(exe, tmp_path, env_extra=None):
    """{case name: [output lines]} — one run of the driver per distinct set of switches."""
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    base.update(env_extra or {})
    groups, out = {}, {}
    for name, env, b in cases():
        groups.setdefault(tuple(sorted(env.items())), []).append((name, b))
    for gi, (env, members) in enumerate(groups.items()):
        files = []
        for k, (name, b) in enumerate(members):
            p = tmp_path / ("g%d_%d.bin" % (gi, k))
            if not p.exists():
                p.write_bytes(b)
            files.append(str(p))
        r = subprocess.run([str(exe)] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(base, **dict(env)), timeout=600)
        text = r.stdout.decode(errors="replace")
        assert r.returncode == 0, text[-3000:]
        parts = text.split("== ")[1:]
        assert len(parts) == len(members), text[-3000:]
        for (name, _), part in zip(members, parts):
            out[name] = part.splitlines()[1:]
    return out
