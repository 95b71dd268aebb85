"""The wide-counter model (tests/wide_counter_model.py, the checker of tests/test_gpu_wide_counters.py) against the
genuine reference: CountingBloomFilter<uint16_t / uint32_t / uint64_t> compiled behind
tests/cpp/ref_wide_counter_driver.cpp from where the reference's headers lie.

The reference's outputs on the seeded cases are pinned in tests/golden/wide_counter_vs_ref.json (digests of the body, of
insertAndCheck's answers, of the minimum counts and of the stored file, popCount / filtered_popcount, and the figures
the conditions below are asserted on) and, for the 8-byte and 1000-byte filters, as stored files
tests/golden/wcbf_*.bf, so the tests run everywhere; where the reference tree is present the driver is built and
compared live as well.  The pins were recorded from the reference build, never from the model, with
    BTLBF_RECORD_REF_GOLDEN=1 python -m pytest tests/test_wide_counter_vs_ref.py

Conditions on the reference's own output, so that no case passes vacuously (figures of wide_counter_model.figures):
per width at least one case leaves a counter > 255 and at least one saturates a counter at MAX that was below it; for
16 bits at least one case changes both halves of one 32-bit word; in every case of the 1000-byte filter (500 / 250 /
125 counters, no power of two) at least one probe's `% counters` and `% bytes` positions differ; every prefilled case of
incrementAll or insert on the 1000- and 4096-byte filters with h >= 3 crosses 255 -> 256 in some counter; on the 8-byte
16-bit filter incrementAll raises a counter whose neighbour in the word stands at 0xffff, and the neighbour stays."""
import json
import os
import subprocess

import numpy as np
import pytest
from conftest import GOLDEN, ROOT, load_golden

import wide_counter_model as wm

GOLDEN_FILE = "wide_counter_vs_ref.json"
RECORD = bool(os.environ.get("BTLBF_RECORD_REF_GOLDEN"))
REF_DIR = os.environ.get("BTLBF_REFERENCE_DIR", "/root/reference")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the reference driver, built where the reference tree lies; None elsewhere"""
    if not os.path.exists(os.path.join(REF_DIR, "CountingBloomFilter.hpp")):
        if RECORD:
            pytest.fail("recording needs the reference tree")
        return None
    exe = str(tmp_path_factory.mktemp("refwide") / "ref_wide_counter_driver")
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++11", "-O1", "-w", "-fno-access-control", "-I" + REF_DIR,
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "ref_wide_counter_driver.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def live(driver, tmp_path_factory):
    """{case key: the driver's output of the case} of one run over all cases; None without the reference"""
    if not driver:
        return None
    d = tmp_path_factory.mktemp("refwide_io")
    lines = []
    for shape, bits, op in wm.CASES:
        nbytes, h, k, thr, reads, body = wm.make_case(shape, bits)
        lines.append("%d %d %d %d %d %s %d %s" % (bits, nbytes, h, k, thr, op, len(reads), body.hex() if any(body) else "-"))
        lines += [s.decode() for s in reads]
    (d / "in.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, str(d / "in.txt"), str(d / "out.bf")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == 7 * len(wm.CASES)
    res = {}
    for i, (shape, bits, op) in enumerate(wm.CASES):
        f = dict(ln.split(" ", 1) for ln in out[7 * i: 7 * i + 7])
        res[wm.case_key(shape, bits, op)] = {
            "size": [int(x) for x in f["size"].split()], "body": bytes.fromhex(f["body"]),
            "out": [] if f["out"] == "-" else [int(c) for c in f["out"]], "min": [int(x) for x in f["min"].split()],
            "pop": [int(x) for x in f["pop"].split()], "file": bytes.fromhex(f["file"]), "reload": int(f["reload"])}
    return res


@pytest.fixture(scope="module")
def table():
    t = {} if RECORD else load_golden(GOLDEN_FILE)
    yield t
    if RECORD:
        with open(os.path.join(GOLDEN, GOLDEN_FILE), "w") as f:
            json.dump(dict(sorted(t.items())), f, indent=1)
            f.write("\n")


def digest_list(xs):
    return wm.sha(json.dumps([int(x) for x in xs]).encode())


@pytest.mark.parametrize("shape,bits,op", wm.CASES, ids=[wm.case_key(*c) for c in wm.CASES])
def test_model_against_reference(oracle, live, table, shape, bits, op):
    key = wm.case_key(shape, bits, op)
    nbytes, h, k, thr, reads, before = wm.make_case(shape, bits)
    assert any(b"N" in s for s in reads) and any(len(s) < k for s in reads) and reads[0] == reads[4]
    f, out, rows = wm.run_model(oracle, shape, bits, op)
    mins = [f.min_count(r) for r in rows]
    commit = wm.SHAPES[shape][7] and op in ("min", "all")
    if live:
        e = live[key]
        if RECORD:
            table[key] = {"size": e["size"], "body_sha": wm.sha(e["body"]), "out_sha": digest_list(e["out"]),
                          "min_sha": digest_list(e["min"]), "pop": e["pop"], "file_sha": wm.sha(e["file"]),
                          "figures": wm.figures(bits, before, e["body"], rows, e["size"][0], e["size"][1])}
            if commit:
                with open(os.path.join(GOLDEN, wm.fixture_name(shape, bits, op)), "wb") as fh:
                    fh.write(e["file"])
        assert e["reload"] == 1
        assert [f.size, f.size_bytes] == e["size"]
        assert f.body() == e["body"], key
        assert out == e["out"] and mins == e["min"], key
        assert [f.pop_count(), f.filtered_popcount()] == e["pop"]
        assert f.file_bytes() == e["file"], key
    pin = table[key]
    assert [f.size, f.size_bytes] == pin["size"]
    assert f.size * (bits // 8) == f.size_bytes
    assert wm.sha(f.body()) == pin["body_sha"], key
    assert digest_list(out) == pin["out_sha"] and digest_list(mins) == pin["min_sha"], key
    assert [f.pop_count(), f.filtered_popcount()] == pin["pop"]
    assert wm.sha(f.file_bytes()) == pin["file_sha"], key
    if commit:  # the committed file is the reference's file
        data = open(os.path.join(GOLDEN, wm.fixture_name(shape, bits, op)), "rb").read()
        assert wm.sha(data) == pin["file_sha"] and data == f.file_bytes()
    print(key, pin["figures"])
    over255, saturated, both, differ = pin["figures"]
    if shape.startswith("c1000"):
        assert differ >= 1, key
    if shape in ("c1000", "c1000h5", "c4096") and op in ("min", "all"):  # (the 8-byte filter has too few counters for all)
        b = np.frombuffer(before, wm.DTYPES[bits])
        a = np.frombuffer(f.body(), wm.DTYPES[bits])
        assert ((b == 0xff) & (a >= 0x100)).any(), key  # the carry inside the counter
    if shape == "c8" and bits == 16 and op == "all":  # 0xffff beside a counter that is incremented: no carry into it
        b = np.frombuffer(before, wm.DTYPES[16]).reshape(-1, 2)
        a = np.frombuffer(f.body(), wm.DTYPES[16]).reshape(-1, 2)
        assert (((b[:, 0] == 0xffff) & (a[:, 1] > b[:, 1])) | ((b[:, 1] == 0xffff) & (a[:, 0] > b[:, 0]))).any()
        assert ((b == 0xffff) <= (a == 0xffff)).all()


@pytest.mark.parametrize("bits", [16, 32, 64])
def test_conditions_hold_on_the_reference_output(table, bits):
    """after the cases above (which fill the table when recording)"""
    figs = [v["figures"] for k, v in table.items() if "_u%d_" % bits in k]
    assert figs
    assert sum(f[0] for f in figs) >= 1 and sum(f[1] for f in figs) >= 1
    if bits == 16:
        assert sum(f[2] for f in figs) >= 1
