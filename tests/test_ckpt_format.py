"""The checkpoint file's framing (csrc/ckpt_format.h) on the CPU: tests/ckpt_format_main.cpp, built with the host
compiler, run as a child process on files written here and checked against tests/ckpt_format_ref.py (an
independent restatement from the format comment): every verdict and every reported offset and length.  The same
program is built and run once more under AddressSanitizer + UndefinedBehaviorSanitizer (-fno-sanitize-recover: any
finding aborts it); that binary runs directly, nothing of it is loaded into Python."""
import itertools
import json
import os
import struct
import subprocess

import pytest

import ckpt_format_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "ckpt_format_main.cpp")
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
FLUID = ref.fluid_part(4, 3)  # 4 x 3, f64, no points: 152 + 9 * 12 * 8 bytes
PAYLOAD = {ref.SCALAR: bytes(range(40)), ref.TRACERS: b"", ref.AVERAGE: bytes(range(7))}  # any bytes: never looked into


def build(out, flags):
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", *flags, "-o", str(out), SRC]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(out)


def runner(exe):
    def run(lines):
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=e)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        out = [json.loads(ln) for ln in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


@pytest.fixture(scope="module")
def scanner(tmp_path_factory):
    return runner(build(tmp_path_factory.mktemp("ckpt_format") / "ckpt_format", ["-O2"]))


def cases():
    """(name, file bytes): the fluid part of FLUID followed by each observer part under test."""
    sec = lambda k: ref.section(k, PAYLOAD.get(k, b""))
    end = ref.section(ref.END)
    out = [("fluid only", FLUID)]
    for n in range(4):
        for subset in itertools.combinations((ref.SCALAR, ref.TRACERS, ref.AVERAGE), n):
            out.append(("subset %s" % (subset,), FLUID + b"".join(sec(k) for k in subset) + end))
    out += [
        ("no end section", FLUID + sec(ref.SCALAR) + sec(ref.AVERAGE)),
        ("unknown tag", FLUID + sec(ref.SCALAR) + ref.section(ref.TRACERS, b"abc", tag=b"IBLBXYZ1") + end),
        ("version of a tag that is not known", FLUID + ref.section(ref.SCALAR, b"abc", tag=b"IBLBSCL2") + end),
        ("out of order", FLUID + sec(ref.TRACERS) + sec(ref.SCALAR) + end),
        ("average before tracers", FLUID + sec(ref.AVERAGE) + sec(ref.TRACERS) + end),
        ("duplicated", FLUID + sec(ref.SCALAR) + sec(ref.SCALAR) + end),
        ("two end sections", FLUID + sec(ref.SCALAR) + end + end),
        ("a section after the end", FLUID + end + sec(ref.SCALAR)),
        ("length past the file", FLUID + ref.section(ref.SCALAR, PAYLOAD[ref.SCALAR], length=41 + 16) + end),
        ("length past the file by one", FLUID + ref.section(ref.AVERAGE, PAYLOAD[ref.AVERAGE], length=8)),
        ("huge length", FLUID + ref.section(ref.SCALAR, PAYLOAD[ref.SCALAR], length=2**62) + end),
        ("negative length", FLUID + ref.section(ref.SCALAR, PAYLOAD[ref.SCALAR], length=-1) + end),
        ("most negative length", FLUID + ref.section(ref.TRACERS, b"", length=-2**63) + end),
        ("end section with a payload", FLUID + sec(ref.SCALAR) + ref.section(ref.END, b"12345678")),
        ("bytes after the end", FLUID + sec(ref.SCALAR) + end + b"\0"),
        ("sixteen bytes after the end", FLUID + end + bytes(16)),
        ("shorter than the fluid part", FLUID[:-1]),
        ("empty file", b""),
    ]
    return out


def check(scanner, tmp_path, named):
    paths = []
    for n, (_, data) in enumerate(named):
        p = tmp_path / ("f%04d.ck" % n)
        p.write_bytes(data)
        paths.append(p)
    got = scanner(["scan %d %s" % (len(FLUID), p) for p in paths])
    for (name, data), o in zip(named, got):
        verdict, found = ref.scan(data, len(FLUID))
        assert o["status"] == verdict, (name, o)
        assert o["size"] == len(data), name
        assert o["present"] == [int(k in found) for k in range(4)], (name, o)
        assert o["offset"] == [found.get(k, (0, 0))[0] for k in range(4)], (name, o)
        assert o["length"] == [found.get(k, (0, 0))[1] for k in range(4)], (name, o)
        assert o["observers"] == ref.observers(found), (name, o)
    return got


def test_the_restatement_knows_the_verdicts():
    """The cases cover every verdict but the I/O one, so a scanner that agreed with a restatement that accepted
    everything would not pass."""
    want = {"fluid only": ref.OK, "no end section": ref.NO_END, "unknown tag": ref.TAG, "out of order": ref.ORDER,
            "duplicated": ref.ORDER, "two end sections": ref.TRAILING, "a section after the end": ref.TRAILING,
            "length past the file": ref.LENGTH, "length past the file by one": ref.LENGTH, "huge length": ref.LENGTH,
            "negative length": ref.LENGTH, "most negative length": ref.LENGTH, "end section with a payload": ref.LENGTH,
            "bytes after the end": ref.TRAILING, "shorter than the fluid part": ref.FLUID_SHORT,
            "empty file": ref.FLUID_SHORT}
    seen = {name: ref.scan(data, len(FLUID))[0] for name, data in cases()}
    for name, v in want.items():
        assert seen[name] == v, name
    assert sum(v == ref.OK for n, v in seen.items() if n.startswith("subset")) == 8


def test_every_case(scanner, tmp_path):
    got = check(scanner, tmp_path, cases())
    full = [o for (name, _), o in zip(cases(), got) if name == "subset (0, 1, 2)"][0]
    at = len(FLUID)
    assert full["offset"] == [at + 16, at + 16 + 40 + 16, at + 16 + 40 + 16 + 16, at + 16 + 40 + 16 + 16 + 7 + 16]
    assert full["length"] == [40, 0, 7, 0] and full["observers"] == 7


def test_truncation_at_every_byte(scanner, tmp_path):
    """A two-section file cut at every offset from the fluid part's end on: valid only whole, or cut back to the
    fluid part."""
    whole = FLUID + ref.section(ref.SCALAR, PAYLOAD[ref.SCALAR]) + ref.section(ref.AVERAGE, PAYLOAD[ref.AVERAGE]) + \
        ref.section(ref.END)
    cuts = list(range(len(FLUID) - 2, len(whole) + 1))
    got = check(scanner, tmp_path, [("cut at %d" % n, whole[:n]) for n in cuts])
    ok = [n for n, o in zip(cuts, got) if o["status"] == ref.OK]
    assert ok == [len(FLUID), len(whole)]


def test_the_fluid_header_gives_the_fluid_part_its_length(scanner, tmp_path):
    files = {
        "f64": ref.fluid_part(4, 3, t=11),
        "f32 with points": ref.fluid_part(5, 2, prec=1, t=3, ns=7),
        "cilia": ref.fluid_part(4, 3, t=5, ns=96, cilia=1, c_num=1),
        "slab": ref.fluid_part(8, 3, ncol=3, x_begin=5, t=2),
    }
    bad = {
        "magic": b"IBLBCK02" + files["f64"][8:],
        "version": files["f64"][:8] + struct.pack("<q", 2) + files["f64"][16:],
        "no rows": ref.fluid_part(4, 0),
        "slab outside": ref.fluid_part(8, 3, ncol=3, x_begin=6),
        "precision": ref.fluid_part(4, 3, prec=2),
        "negative step": ref.fluid_part(4, 3, t=-1),
        "negative points": files["f64"][:8 + 7 * 8] + struct.pack("<q", -1) + files["f64"][8 + 8 * 8:],
        "short header": files["f64"][:100],
    }
    names = list(files) + list(bad)
    for n, name in enumerate(names):
        (tmp_path / ("h%d.ck" % n)).write_bytes(files.get(name, bad.get(name)) + ref.section(ref.TRACERS, b"xy") +
                                                 ref.section(ref.END))
    got = scanner(["info %s" % (tmp_path / ("h%d.ck" % n)) for n in range(len(names))])
    for name, o in zip(names, got):
        if name in files:
            assert o["fluid"] == len(files[name]), (name, o)
            assert o["status"] == ref.OK and o["observers"] == 2 and o["offset"][ref.TRACERS] == len(files[name]) + 16
            assert o["step"] == struct.unpack("<q", files[name][8 + 6 * 8:8 + 7 * 8])[0]
        else:
            assert o["fluid"] == -1, (name, o)


def test_under_the_sanitizers(tmp_path):
    """The same program under ASan + UBSan on every case above and every truncation: it must end clean."""
    run = runner(build(tmp_path / "ckpt_format_san", SAN_FLAGS))
    check(run, tmp_path, cases())
    test_truncation_at_every_byte(run, tmp_path)
    test_the_fluid_header_gives_the_fluid_part_its_length(run, tmp_path)
