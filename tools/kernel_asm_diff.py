"""Is the device code of two source trees the same, kernel by kernel?  (no GPU needed: hipcc cross-compiles)
Every unit of build.units() is compiled to gfx950 assembly in both trees with that tree's own build.FLAGS and -D flags, split per
function symbol and compared: the set of kernels, every instruction stream and every .amdhsa_kernel descriptor (registers, scratch,
LDS, occupancy inputs).  Only what depends on a function's POSITION in its unit is normalised: the __hip_cuid_<hash> symbol, the
function index in local labels (.LBB<n>_<m>, .Lfunc_end<n>, .Ltmp<n>), compiler comments and the order of the functions.
usage: python tools/kernel_asm_diff.py <parent-tree> <this-tree>      exit status 0 = identical, 1 = any difference"""
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile


def load_build(tree):
    spec = importlib.util.spec_from_file_location("cagym_build_" + re.sub(r"\W", "_", tree), os.path.join(tree, "gym-exploration-2d_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(job):
    b, obj, src, defs = job
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, obj + ".s")
        cmd = [os.environ.get("HIPCC", "hipcc"), "--offload-arch=" + b.ARCH, "--cuda-device-only", "-S"] + b.FLAGS + defs + ["-o", out, os.path.join(b.CSRC, src)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode:
            raise RuntimeError("%s: %s failed\n%s" % (b.CSRC, obj, p.stderr))
        return obj, open(out).read()


def normalise(lines):
    tmp = {}
    out = []
    for line in lines:
        line = line.split(";")[0].rstrip()  # compiler comments name basic blocks by function index
        if not line:
            continue
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", line)
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
        line = re.sub(r"(\.L[A-Za-z]+)\d+_(\d+)", r"\1_\2", line)
        line = re.sub(r"\.Ltmp\d+", lambda m: tmp.setdefault(m.group(0), ".Ltmp%d" % len(tmp)), line)
        out.append(line)
    return out


def split(text):
    """{symbol: (is_kernel, instruction lines, descriptor lines)} of one unit's assembly"""
    funcs = {}
    lines = text.splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if not m:
            i += 1
            continue
        sym = m.group(1)
        j = i + 1
        while not re.match(r"\.Lfunc_end\d+:", lines[j]):
            j += 1
        body, desc, in_desc = [], [], False
        for line in lines[i + 1:j]:
            if re.match(r"\s*\.amdhsa_kernel\s", line):
                in_desc = True
            (desc if in_desc else body).append(line)
            if re.match(r"\s*\.end_amdhsa_kernel", line):
                in_desc = False
        funcs[sym] = (bool(desc), normalise(body), normalise(desc))
        i = j + 1
    return funcs


def first_difference(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "line %d: %r != %r" % (k, x, y)
    return "length %d != %d" % (len(a), len(b))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    builds = [load_build(os.path.abspath(t)) for t in sys.argv[1:]]
    units = [[(o, s, d) for (o, s, d, _h) in b.units()] for b in builds]
    bad = 0
    if [u[0] for u in units[0]] != [u[0] for u in units[1]]:
        print("the trees build different units: %s != %s" % ([u[0] for u in units[0]], [u[0] for u in units[1]]))
        bad += 1
    jobs = [(b, o, s, d) for b, us in zip(builds, units) for (o, s, d) in us]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(jobs), int(os.environ.get("MAX_JOBS") or os.cpu_count() or 2))) as ex:
        res = list(ex.map(assemble, jobs))
    parent, this = dict(res[:len(units[0])]), dict(res[len(units[0]):])
    for obj in [u[0] for u in units[0] if u[0] in this]:
        fa, fb = split(parent[obj]), split(this[obj])
        diffs = ["%s only in %s" % (s, sys.argv[1] if s in fa else sys.argv[2]) for s in sorted(set(fa) ^ set(fb))]
        for s in sorted(set(fa) & set(fb)):
            for what, x, y in (("instructions", fa[s][1], fb[s][1]), ("descriptor", fa[s][2], fb[s][2])):
                if x != y:
                    diffs.append("%s: %s differ, %s" % (s, what, first_difference(x, y)))
        print("%-18s %3d kernels, %d other functions, %7d instruction lines: %s" % (
            obj, sum(f[0] for f in fa.values()), sum(not f[0] for f in fa.values()), sum(len(f[1]) for f in fa.values()),
            "DIFFERENT" if diffs else "identical"))
        for d in diffs:
            print("    " + d)
        bad += len(diffs)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
