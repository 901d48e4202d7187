"""CPU: the visitors of csrc/cagym_layout.h, which turn ONE listing of a block's members into the allocation's size, the members'
pointers and the entries of a checkpoint table (cagym_api.hip builds the stream, log, replay and trajectory blocks with them),
compiled by the host compiler with the address and undefined-behaviour sanitizers (tests/layout_check.cpp, a stand-alone program):

  - every order of an 8-byte, a 4-byte, a 1-byte member and one member no checkpoint carries, with the counts 0, 1, 3 and 1000;
  - the byte sum is the last member's end rounded up to 16; every pointer is 16-aligned and inside the block; no two members overlap;
    every element is written and read back in an allocation of exactly that size;
  - the checkpoint entries are the flagged members, in order, at ascending multiples of 16, with bytes = sizeof(T) * count;
  - the sizes-only pass over an empty struct gives the same offsets with null bases."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_layout_visitors(tmp_path):
    exe = str(tmp_path / "layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "gym-exploration-2d_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "layout_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"layout_check ok: (\d+) cases", out.stdout)
    assert m and int(m.group(1)) == 24 * 256
