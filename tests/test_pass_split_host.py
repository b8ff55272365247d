"""CPU: what the pooled passes do on the host with their survivors (pyfaceanalysis_amd/csrc/hg_frame_list.hpp — the split of the
survivors by frame, the bounds of a pooled eye tail's segment words and the layout of its rows) in a stand-alone driver with its own
main (tests/pass_split_driver.cpp), built plain and with AddressSanitizer + UndefinedBehaviorSanitizer and run directly, nothing
preloaded, on a few hundred seeded cases against restatements of the functions the header's replaced."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ok(out):
    last = out.strip().splitlines()[-1].split()
    return last[0] == "ok" and int(last[1]) == 402 and int(last[2]) >= 4 * 400


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_split_and_tail_layout_under_asan_ubsan(tmp_path):
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "pyfaceanalysis_amd", "csrc")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    src = os.path.join(ROOT, "tests", "pass_split_driver.cpp")
    # the driver itself must compile and pass as a plain build: a compile error is a failure, never a skip
    plain = tmp_path / "pass_split_driver_plain"
    r = subprocess.run(base + [src, "-o", str(plain)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    r = subprocess.run([str(plain)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and _ok(r.stdout.decode()), r.stdout.decode(errors="replace")[-3000:]
    # only a missing sanitizer runtime is a reason to skip: asked of a trivial program, not of the driver
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        pytest.skip("no sanitizer runtime here: " + r.stdout.decode(errors="replace")[-300:])
    exe = tmp_path / "pass_split_driver"
    r = subprocess.run(base + san + [src, "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
    assert _ok(out), out[-500:]
