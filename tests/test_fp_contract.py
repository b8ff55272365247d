"""CPU: the float64 glue kernels are compiled without fused multiply-adds of their own.  The cascade glue, the rotated-window
coefficients and the eye / purge glue claim numpy's and PIL's bits, one rounding per operation; hipcc's default
-ffp-contract=fast-honor-pragmas fuses a multiply into a following add unless the source says otherwise, and one fused rounding
moves a value that sits on a discard threshold or a 16.16 fixed-point boundary.  Each glue file is compiled to gfx950 assembly
with the build's flags, once as it is and once with -ffp-contract=off; the count of float64 fma instructions (v_fma_f64 and the
accumulating v_fmac_f64) of every glue kernel must not change (the fma that remain are the math library's own, in cos / sin / fmod)."""
import os
import re
import shutil
import subprocess

import pytest

from pyfaceanalysis_amd import build

# file -> kernels whose float64 arithmetic follows numpy / PIL operation by operation (matched by name, templates by prefix)
GLUE = {
    "hg_cascade.hip": ["k_cascade_update", "k_cascade_group", "k_cascade_group_mark", "k_cascade_init_grid"],
    "hg_extract.hip": ["k_extent_tables", "k_extent_gather_rot<"],
    "hg_eyes.hip": ["k_eye_boxes", "k_eyes_glue", "k_purge"],
}


def _fma_counts(path):
    """{demangled kernel name: count of float64 fused multiply-adds (v_fma_f64, v_fmac_f64_e32 / _e64)} of one device assembly file."""
    names, order, cur = {}, [], None
    for line in open(path):
        m = re.match(r"\s*\.type\s+([^,]+),@function", line)
        if m:
            cur = m.group(1)
            order.append(cur)
            names[cur] = 0
        elif cur and re.match(r"\.Lfunc_end\d+:", line):
            cur = None
        elif cur and re.match(r"\s*v_fmac?_f64(_e32|_e64)?\b", line):
            names[cur] += 1
    dem = subprocess.run(["c++filt"], input="\n".join(order), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    return {d.replace("(anonymous namespace)::", "").replace("void ", "", 1): names[o] for o, d in zip(order, dem)}


def _kernels(counts, name):
    if name.endswith("<"):
        return {k: v for k, v in counts.items() if k.startswith(name)}
    return {k: v for k, v in counts.items() if k.startswith(name + "(")}


@pytest.mark.skipif(not os.path.exists(build.HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
@pytest.mark.parametrize("src", sorted(GLUE))
def test_glue_kernels_have_no_contracted_fma(tmp_path, src):
    counts = {}
    for tag, extra in (("built", []), ("off", ["-ffp-contract=off"])):
        out = tmp_path / (tag + ".s")
        cmd = [build.HIPCC] + build.FLAGS + ["-x", "hip", "--cuda-device-only", "-S"] + extra + [os.path.join(build.CSRC, src), "-o", str(out)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
        counts[tag] = _fma_counts(str(out))
    for name in GLUE[src]:
        built, off = _kernels(counts["built"], name), _kernels(counts["off"], name)
        assert built and set(built) == set(off), (src, name, sorted(counts["built"]))
        assert built == off, (src, name, built, off)
