"""CPU: the rank of an OtherAgentsStates row (csrc/cagym_oas_rank.h: a count with 64-bit integer compares on the key bits, and the fp64
definition for every lane of a wave in which some lane's key is negative or has an exact tie), compiled by the host compiler and
held to the definition  before(j) = #{ l : kl > kj or (kl == kj and l > j) }  (tests/oas_rank_check.cpp):

  - every row of 4 keys over {-inf, a negative, +0, a positive, a tied value}, each alone in its wave and all of them packed;
  - 1.6 million random rows of 10 and 20 keys with -inf padding, injected exact ties, negative keys, subnormals and keys of every
    exponent, ranked 64 lanes at a time, the fast and the fallback path selected as the kernel selects them.

NaN and -0 are not among the inputs: the pair phase cannot produce them (the header says why)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_integer_rank_and_fallback_agree_with_the_definition(tmp_path):
    exe = str(tmp_path / "oas_rank_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "gym-exploration-2d_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "oas_rank_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "oas_rank_check ok" in out.stdout
    m = re.search(r"rows (\d+) fast waves (\d+) exact waves (\d+)", out.stdout)
    assert int(m.group(1)) >= 10 ** 6 and int(m.group(2)) > 1000 and int(m.group(3)) > 1000
