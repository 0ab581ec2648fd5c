"""CPU: the owner of every device block of the library (webdgs_amd/csrc/devmem.h) against a counting wdgs_alloc / wdgs_free that can fail on request --
each block freed exactly once across destruction, reset, moves and self-move; free before request on re-allocation; an EMPTY handle (no pointer, no
count) after a failed allocation; release / adopt without a free; a struct of three handles refilled with the second allocation failing.  The class is
plain C++: built here with g++, no GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devmem_ownership(tmp_path):
    exe = os.path.join(tmp_path, "devmem_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "devmem_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "devmem: ok" in r.stdout, r.stdout + r.stderr
