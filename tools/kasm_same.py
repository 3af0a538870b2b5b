#!/usr/bin/env python3
"""Development: is the product library's device code the same in two source trees?

Compiles the translation units of the library (cal_22-mpc_amd/build.py: lib_units) to gfx950 device assembly
(hipcc -O3 -S --cuda-device-only, MPC_TESTING=0) from this tree's csrc and from another tree's (a worktree of the parent
commit), cuts the assembly into its functions and prints one line per kernel: the compiler's own figures behind the
function ("; codeLenInByte", "; NumVgprs", ...) and whether the function's text is the same in both trees.  The
__hip_cuid_<hash> symbol, a hash of the compilation, is left out of the comparison.  Exit status 1 if anything differs.

    tools/kasm_same.py OTHER_CSRC [--units kernels,baselines,sizes,lane_w8,lane_w16,lane_w32] [--save profiles/x.txt]
"""
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("mpc_build", os.path.join(ROOT, "cal_22-mpc_amd", "build.py"))
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)

args = sys.argv[1:]
save, want = None, "kernels,baselines,sizes,lane_w8,lane_w16,lane_w32"
if "--save" in args:
    i = args.index("--save"); save = args[i + 1]; del args[i:i + 2]
if "--units" in args:
    i = args.index("--units"); want = args[i + 1]; del args[i:i + 2]
other = os.path.abspath(args[0])
want = want.split(",")

FIGURES = [("codeLenInByte", "code bytes"), ("NumVgprs", "VGPRs"), ("NumAgprs", "AGPRs"), ("ScratchSize", "scratch"),
           ("LDSByteSize", "LDS"), ("Occupancy", "occupancy")]


def functions(path):
    """{symbol: (text, figures)} of one assembly file, in the file's order."""
    text = re.sub(r"__hip_cuid_\w+", "__hip_cuid", open(path).read())
    parts = re.split(r"(?m)^\s*\.type\s+(\S+),@function\s*$", text)
    out = {}
    for name, body in zip(parts[1::2], parts[2::2]):
        fig = {k: (re.search(r";\s*%s\s*[:=]\s*(\d+)" % k, body) or [None, "?"])[1] for k, _ in FIGURES}
        out[name] = (body, fig)
    return out


with tempfile.TemporaryDirectory() as td:
    jobs = []
    for tree, csrc in (("here", build.CSRC), ("other", other)):
        for src, obj, extra in build.lib_units(csrc):
            unit = obj[:-2]
            if unit not in want:
                continue
            asm = os.path.join(td, f"{tree}_{unit}.s")
            cmd = [build.HIPCC, *build.FLAGS, *extra, "-S", "--cuda-device-only", src, "-o", asm]
            jobs.append((cmd, subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True)))
    for cmd, p in jobs:
        err = p.communicate()[1]
        if p.returncode:
            sys.stderr.write(err[-4000:])
            raise SystemExit(p.returncode)
    filt = shutil.which("llvm-cxxfilt", path=os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin")) or "c++filt"
    rows, differ = [], 0
    for unit in want:
        a, b = functions(os.path.join(td, f"here_{unit}.s")), functions(os.path.join(td, f"other_{unit}.s"))
        names = list(a) + [n for n in b if n not in a]
        plain = subprocess.run([filt] + names, capture_output=True, text=True).stdout.split("\n") if names else []
        for n, d in zip(names, plain):
            same = n in a and n in b and a[n][0] == b[n][0]
            differ += 0 if same else 1
            fig = (a.get(n) or b[n])[1]
            if fig["codeLenInByte"] == "?":                 # a device function that is not a kernel
                continue
            short = re.sub(r"\(anonymous namespace\)::", "", d or n).split("(")[0].replace("void ", "")
            rows.append(f"{unit:<10}" + "".join(f"{fig[k]:>11}" for k, _ in FIGURES) + f"  {'yes' if same else 'NO':<5} {short}")

head = (f"# tools/kasm_same.py: device assembly ({' '.join(build.FLAGS)} -S --cuda-device-only) of this tree and of another\n"
        f"# {'unit':<8}" + "".join(f"{t:>11}" for _, t in FIGURES) + "  same  kernel\n")
text = (head + "\n".join(rows) + f"\n# {len(rows)} kernels, {differ} functions differ\n"
        "# (a name left mangled is one the demangler cannot read: a kernel with an empty template parameter pack, such as\n"
        "# vpc_lane_kernel<W, with per-line outputs> without a module sequence, the run-time loop)\n")
print(text, end="")
if save:
    with open(save, "w") as f:
        f.write(text)
raise SystemExit(1 if differ else 0)
