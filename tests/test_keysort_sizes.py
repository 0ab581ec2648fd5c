"""CPU: the sizing rule of the stable u64 key sort (webdgs_amd/csrc/keysort_sizes.h) -- tile, workgroups and table words at the sizes where the tiling
changes, up to the largest size a caller may pass; a table that is not monotone in the size; the three sizes a sort reserves for two users' sizes.  The
header is plain C++: built here with g++, no GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keysort_sizes(tmp_path):
    exe = os.path.join(tmp_path, "keysort_sizes_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "keysort_sizes_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "keysort_sizes: ok" in r.stdout, r.stdout + r.stderr
