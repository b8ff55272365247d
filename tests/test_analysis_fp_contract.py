"""CPU: the age-patch kernels are compiled without fused multiply-adds of their own — the method of tests/test_fp_contract.py on
hg_estimate.hip.  k_age_patch claims PIL's coordinate and filter arithmetic and the eye step's contrast arithmetic, one rounding per
operation; its count of float64 fma instructions must be the same with -ffp-contract=off (every filter's instantiation), and so must
that of the composed path's contrast kernel."""
import os
import shutil
import subprocess

import pytest

from pyfaceanalysis_amd import analysis, build      # noqa: F401  (analysis: the module this file's kernels serve)
from tests.test_fp_contract import _fma_counts, _kernels

SRC = "hg_estimate.hip"
KERNELS = ["k_age_patch<", "k_patch_contrast"]


@pytest.mark.skipif(not os.path.exists(build.HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_patch_kernels_have_no_contracted_fma(tmp_path):
    assert SRC in build.SOURCES
    counts = {}
    for tag, extra in (("built", []), ("off", ["-ffp-contract=off"])):
        out = tmp_path / (tag + ".s")
        cmd = [build.HIPCC] + build.FLAGS + ["-x", "hip", "--cuda-device-only", "-S"] + extra + [os.path.join(build.CSRC, SRC), "-o", str(out)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
        counts[tag] = _fma_counts(str(out))
    for name in KERNELS:
        built, off = _kernels(counts["built"], name), _kernels(counts["off"], name)
        assert built and set(built) == set(off), (name, sorted(counts["built"]))
        assert built == off, (name, built, off)
    assert len(_kernels(counts["built"], "k_age_patch<")) == 3      # NEAREST, BILINEAR, BICUBIC
