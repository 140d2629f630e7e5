"""CPU check of the composite stage's arrival arithmetic (easyhec_amd/csrc/ehr_arrive.h): the finisher waits until every
XCD's counter has reached the number vb_comp_expected gives, so a count that is off by one either holds the step until the
bounded wait reports it or lets the finish run before the last sums have landed.  tests/native/comp_arrivals_check.cpp
compares the header's numbers with a brute-force count over every launch shape with nitems 0..200 and 1 / 2 / 3 / 24
workgroups per XCD, with and without zero-fill tiles and link boxes."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "comp_arrivals_check.cpp")


def _compiler():
    for name in ("g++", "c++", "clang++"):
        p = shutil.which(name)
        if p:
            return p
    for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(p):
            return p
    return None


def test_comp_arrivals_brute_force(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler found (the library itself needs hipcc, which ships clang++)"
    exe = str(tmp_path / "comp_arrivals_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    # 4 counts of workgroups x 201 item counts x 6 fills x 6 box counts x 8 XCDs
    assert int(out.stdout.split()[1]) == 4 * 201 * 36 * 8
