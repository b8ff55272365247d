"""CPU: the host-only part of the frame-list pass (pyfaceanalysis_amd/csrc/hg_frame_list.hpp — what a list is refused for, first[], the
distinct grids, the rows of the shared tables, the key of the whole list) in a stand-alone driver with its own main
(tests/frame_list_driver.cpp), built with AddressSanitizer + UndefinedBehaviorSanitizer and run on a few hundred seeded lists."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_list_layout_under_asan_ubsan(tmp_path):
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "pyfaceanalysis_amd", "csrc")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    src = os.path.join(ROOT, "tests", "frame_list_driver.cpp")
    # the driver itself must compile and pass as a plain build: a compile error is a failure, never a skip
    plain = tmp_path / "frame_list_driver_plain"
    r = subprocess.run(base + [src, "-o", str(plain)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    r = subprocess.run([str(plain)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and r.stdout.decode().strip().splitlines()[-1].startswith("ok 400 "), r.stdout.decode(errors="replace")[-3000:]
    # only a missing sanitizer runtime is a reason to skip: asked of a trivial program, not of the driver
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        pytest.skip("no sanitizer runtime here: " + r.stdout.decode(errors="replace")[-300:])
    exe = tmp_path / "frame_list_driver"
    r = subprocess.run(base + san + [src, "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
    last = out.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) == 400 and int(last[2]) >= 27 * 20, out[-500:]
