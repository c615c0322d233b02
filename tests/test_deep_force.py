"""The force axis of the deep sweep's collide on the CPU: deep_plan.h's deep_force_x_only and the
IBLB_DEEP_FORCE word, and the facts about make_kforce's constants (iblb_device.h) that the x-only build
(relax_cells / relax_dev with XF) leans on.  tests/deep_force_main.cpp is compiled host-only under
AddressSanitizer + UndefinedBehaviorSanitizer (the flags of oracle/Makefile.san; through hipcc, since
iblb_device.h includes the HIP headers; the program makes no HIP call) and run as a child process.  Any
sanitizer finding aborts the program (-fno-sanitize-recover).

With F_y = +-0 the x-only build reads -hE[2] for hE[3] and -gO[2] for gO[3], and leaves hFy, hE[1] and
gO[1] out.  So for F_x in {0, +-1e-6, +-3.3e-3, 1e-300} x F_y in {+0, -0}, in both compute types:
hFy, hE[1], gO[1] are zeros; hE[2] and gO[2] are F_x kwi4[1] and F_x kwi2[1] (the product taken here
with numpy, in the compute type); hE[3] and gO[3] are -hE[2] and -gO[2].  All compared as bit patterns,
with one exception that IEEE arithmetic forces: where the compute type's F_x is zero (0, and 1e-300 in
float) every constant is a zero, and (F_y - F_x) c = (+0) c = +0 at F_y = +0 while -((F_x + F_y) c) = -0,
so the two zeros differ in their sign bit (hE[3] 0x0, -hE[2] 0x8000000000000000).  There the test asks
for two zeros; the sign of a zero addend beside a nonzero term changes no population (iblb_device.h,
relax_cells), and tests/test_gpu_deep_force.py checks the populations for the force (0, 0) bit for bit.
"""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "deep_force_main.cpp")
CSRC = os.path.join(REPO, "cuda_iblb_11_amd", "csrc")
SAN = os.path.join(REPO, "oracle", "_san", "deep_force_san")
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TAUS = [(0.8, 1.0), (0.51, 0.7), (3.0, 0.55)]
FX = [0.0, 1e-6, -1e-6, 3.3e-3, -3.3e-3, 1e-300]
FY = [0.0, -0.0]


def hx(v):
    return "%x" % struct.unpack("<Q", struct.pack("<d", v))[0]


@pytest.fixture(scope="module")
def prog():
    deps = [SRC, os.path.join(CSRC, "deep_plan.h"), os.path.join(CSRC, "iblb_device.h")]
    if not os.path.exists(SAN) or os.path.getmtime(SAN) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SAN), exist_ok=True)
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
               "-Wall", "-fno-omit-frame-pointer"]
        for f in SAN_FLAGS:
            cmd += ["-Xarch_host", f]
        r = subprocess.run(cmd + ["-o", SAN, SRC], capture_output=True, text=True, cwd=REPO)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([SAN], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=e)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        out = [json.loads(ln) for ln in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def test_x_only(prog):
    """True exactly for F_y = +0 and -0, whatever F_x: a denormal, a NaN or any nonzero F_y is general."""
    nan, inf, den = float("nan"), float("inf"), 5e-324
    fxs = [0.0, -0.0, 1e-6, -2e-6, 1e-300, den, nan, inf]
    yes = [0.0, -0.0]
    no = [den, -den, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-320, nan, -nan, 3e-7, -3e-7, 1.0, inf, -inf]
    cases = [(fx, fy, 1) for fx in fxs for fy in yes] + [(fx, fy, 0) for fx in fxs for fy in no]
    out = prog(["xonly %s %s" % (hx(fx), hx(fy)) for fx, fy, _ in cases])
    for (fx, fy, want), o in zip(cases, out):
        assert o["x_only"] == want, (fx, fy, o)


def test_environment_word(prog):
    """IBLB_DEEP_FORCE takes the one word general; anything else is an error and sets nothing."""
    words = ["general", "-", "General", "GENERAL", "general,", ",general", "generalx", "x", "plain", "0", "1", "xonly"]
    out = prog(["word " + w for w in words])
    for w, o in zip(words, out):
        assert (o["ok"], o["general"]) == ((1, 1) if w == "general" else (0, 0)), (w, o)


@pytest.mark.parametrize("f32", [0, 1], ids=["f64", "f32"])
def test_kforce_constants(prog, f32):
    R = np.float32 if f32 else np.float64
    U = np.uint32 if f32 else np.uint64
    sign = U(1) << U(31 if f32 else 63)
    cases = [(t, fx, fy) for t in TAUS for fx in FX for fy in FY]
    out = prog(["kforce %d %s %s %s %s" % (f32, hx(t[0]), hx(t[1]), hx(fx), hx(fy)) for t, fx, fy in cases])
    for (t, fx, fy), o in zip(cases, out):
        k = {n: U(int(v, 16)) for n, v in o.items()}
        val = {n: np.array([b], dtype=U).view(R)[0] for n, b in k.items()}
        Fx = R(fx)
        assert k["Fx"] == np.array([Fx]).view(U)[0] and val["Fy"] == 0.0, (t, fx, fy, o)
        print("KFORCE", "f32" if f32 else "f64", t, fx, fy, {n: o[n] for n in ("hFy", "hE1", "gO1", "hE2", "hE3", "gO2", "gO3")})
        for n in ("hFy", "hE1", "gO1"):
            assert (k[n] & ~sign) == 0, (n, t, fx, fy, o)
        with np.errstate(under="ignore"):
            pE, pO = Fx * val["kwi4"], Fx * val["kwi2"]
        assert k["hE2"] == np.array([pE]).view(U)[0], (t, fx, fy, o)
        assert k["gO2"] == np.array([pO]).view(U)[0], (t, fx, fy, o)
        for a, b in (("hE3", "hE2"), ("gO3", "gO2")):
            if Fx != 0:
                assert k[a] == (k[b] ^ sign), (a, t, fx, fy, o)
            else:  # two zeros, whose signs F_y's sign decides (the docstring above)
                assert (k[a] & ~sign) == 0 and (k[b] & ~sign) == 0, (a, t, fx, fy, o)
                assert (k[a] == (k[b] ^ sign)) == (np.signbit(fy)), (a, t, fx, fy, o)
