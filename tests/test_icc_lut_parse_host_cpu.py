"""The parser and builders of LUT-based ICC profiles (codec-eval_amd/csrc/ce_icc_lut.cpp) in a stand-alone program under
AddressSanitizer and UBSan (tests/cpp/icc_lut_parse_host.cpp), each input in an allocation of exactly its length: every prefix
of every fixture profile and a fixed-seed set of byte mutations aimed at the header, the tag table, the tag's channel counts,
the five mAB offsets, the grid bytes, the precision, the mft table counts and the curve headers.  Each input must come back as
a kind, with no sanitizer report; the inputs the parser accepts must reproduce the numpy restatement
(tests/icc_lut_restatement.py)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_lut_restatement as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL = (0x00, 0x01, 0x02, 0x03, 0x7F, 0x80, 0xFE, 0xFF)
CURVE = np.dtype([("kind", "<i4"), ("ftype", "<u4"), ("count", "<u4"), ("first", "<u4"), ("q", "<f8", 7)])
KINDS = {"identity": 0, "sampled": 1, "power": 2}


@pytest.fixture(scope="module")
def parse_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("icclutparse") / "icc_lut_parse_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "codec-eval_amd", "csrc", "ce_icc_lut.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "icc_lut_parse_host.cpp"), "-o", str(exe)])
    return str(exe)


def tag_fields(profile: bytes):
    """offsets of the bytes the tag's layout hangs on: its type and channel counts, the five mAB offsets, the CLUT's grid and
    precision bytes, the matrix, each curve element's header and first numbers; for mft* the grid byte and the table counts"""
    n = struct.unpack_from(">I", profile, 128)[0]
    for i in range(n):
        sig, off, size = struct.unpack_from(">4sII", profile, 132 + 12 * i)
        if sig == b"A2B0":
            break
    out = list(range(off, off + 12))
    if profile[off:off + 4] == b"mAB ":
        out += range(off + 12, off + 32)
        ob, omat, om, oc, oa = struct.unpack_from(">5I", profile, off + 12)
        if oc:
            out += range(off + oc, off + oc + 20)
        if omat:
            out += range(off + omat, off + omat + 48)
        for o in (ob, om, oa):
            at = o
            for _ in range(3 if o else 0):
                c, used = L._read_curve(profile[off:off + size], at)
                out += range(off + at, off + at + min(used, 40))
                at += (used + 3) & ~3
    else:
        out += range(off + 8, off + 12)
        out += range(off + 48, off + 52)
    return sorted(set(out))


def inputs():
    F = L.fixtures()
    rng = np.random.default_rng(20250117)
    out = [(name, p) for name, p in sorted(F.items())]
    for name, p in sorted(F.items()):
        out += [(f"{name}[:{k}]", p[:k]) for k in range(len(p))]
    names = sorted(F)
    for i in range(6000):
        name = names[i % len(names)]
        p = bytearray(F[name])
        n_tags = struct.unpack_from(">I", p, 128)[0]
        region = (range(0, 128), range(128, 132 + 12 * n_tags), tag_fields(bytes(p)), tag_fields(bytes(p)))[i // len(names) % 4]
        for _ in range(int(rng.integers(1, 4))):
            at = int(region[int(rng.integers(0, len(region)))])
            p[at] = SPECIAL[int(rng.integers(0, len(SPECIAL)))] if rng.integers(0, 2) else int(rng.integers(0, 256))
        out.append((f"{name}~{i}", bytes(p)))
    return out


def test_every_input_is_answered_and_the_accepted_ones_equal_the_restatement(parse_host, tmp_path):
    cases = inputs()
    with open(tmp_path / "inputs.bin", "wb") as f:
        for _, p in cases:
            f.write(struct.pack("<I", len(p)) + p)
    r = subprocess.run([parse_host, str(tmp_path / "inputs.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout) == len(cases)
    raw = open(tmp_path / "out.bin", "rb").read()
    pos, kinds, accepted_mutants = 0, [0, 0, 0, 0], 0

    def floats(n):
        nonlocal pos
        a = np.frombuffer(raw, np.float32, n, pos)
        pos += 4 * n
        return a

    def u32():
        nonlocal pos
        pos += 4
        return struct.unpack_from("<I", raw, pos - 4)[0]

    for name, p in cases:
        kind = struct.unpack_from("<i", raw, pos)[0]
        pos += 4
        kinds[kind] += 1
        if "[:" in name:
            assert kind == 3, name  # a proper prefix is malformed: the header's size field is past it
        if kind != 0:
            continue
        accepted_mutants += "~" in name
        tables = floats(768).reshape(3, 256)
        clut = floats(u32()).reshape(-1, 4)
        matrix = floats(12)
        curves = np.frombuffer(raw, CURVE, 6, pos)
        pos += 6 * CURVE.itemsize
        samples = floats(u32())
        assert np.array_equal(tables.view(np.uint32), L.input_tables(p, 8).view(np.uint32)), name
        want = L.clut_nodes(p)
        assert clut.size == (want[1].size if want else 0), name
        if want:
            assert np.array_equal(clut.view(np.uint32), want[1].view(np.uint32)), name
        assert np.array_equal(matrix.view(np.uint32), L.matrix12(p).view(np.uint32)), name
        for got, w in zip(curves, L.curves(p)):
            assert got["kind"] == KINDS[w[0]], name
            if w[0] == "sampled":
                assert np.array_equal(samples[got["first"]:got["first"] + got["count"]].view(np.uint32), w[1].view(np.uint32)), name
            if w[0] == "power":
                assert got["ftype"] == w[1] and np.array_equal(got["q"].view(np.uint64), np.array(w[2], np.float64).view(np.uint64)), name
    assert pos == len(raw)
    F = L.fixtures()
    n_prefixes = sum(len(p) for p in F.values())
    # every whole fixture is accepted, every proper prefix refused as malformed, and the mutations reach all four kinds
    assert kinds[0] >= len(F) and kinds[3] >= n_prefixes and all(k > 0 for k in kinds), kinds
    assert accepted_mutants > 100  # a mutation of a field that is not read, or one that leaves a valid layout, is still accepted
    print("kinds", kinds, "accepted mutants", accepted_mutants)
