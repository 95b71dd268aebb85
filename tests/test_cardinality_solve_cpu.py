"""The k-mer cardinality estimate without a GPU: btlbf_card_solve (pure host arithmetic) against the numpy model
(tests/cardinality_model.py), its refusals, the argument errors every btlbf_card_* call reports before any HIP call, and
the accuracy of the sketch's definition itself, measured on the model.

Accuracy input (cardinality_model.accuracy_reads): a genome of 20 000 uniform random bases, 4 096 reads of 100 bases at
random offsets, 1 % substitutions, k = 25: 311 296 windows.  Caps: with sample_bits 0 and table_bits 18, F0 within 2 % and
f1 within 3 % of np.unique (the estimator's standard deviation at this shape is about 0.15 %); with sample_bits 2 and
table_bits 16, F0 within 5 % (the sampling standard deviation is 0.6 %).  Only F0 and f1 get caps: the true f2 is about
a thousand and f3 a few dozen, where the method's errors are tens of percent; those are held to the model instead."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cardinality_model as M
from conftest import ROOT

ptr = lambda a: C.c_void_p(a.ctypes.data)
FAKE = 16  # a handle that is never dereferenced


def lib_solve(lib, t, s, r, poison=0xA5):
    from btl_bloomfilter_amd import _lib as L

    t = np.ascontiguousarray(t, np.uint64)
    est = L.CardEstimate()
    C.memset(C.byref(est), poison, C.sizeof(est))
    f = np.frombuffer(bytes([poison]) * (8 * (t.size - 1)), np.float64).copy()
    rc = lib.btlbf_card_solve(ptr(t), t.size, s, r, C.byref(est), ptr(f))
    return rc, est, f


def close(got, want, F0):
    return abs(got - want) <= 1e-9 * max(abs(want), F0)


def check_against_model(lib, t, s, r):
    from btl_bloomfilter_amd import _lib as L

    want = M.solve(t, s, r)
    assert want is not None
    F0, f, occ = want
    for poison in (0xA5, 0xFF):  # every byte of est and f is written
        rc, est, got = lib_solve(lib, t, s, r, poison)
        assert rc == L.OK, lib.btlbf_last_error()
        assert close(est.distinct, F0, F0) and close(est.singletons, f[1], F0) and close(est.occupancy, occ, 1.0)
        assert (est.windows, est.clean_windows, est.sampled) == (0, 0, 0) and est.overflow_buckets == int(t[-1])
        assert got.size == f.size and got[0] == 0.0
        bad = [i for i in range(f.size) if not close(got[i], f[i], F0)]
        assert not bad, (bad[:5], got[bad[:5]], f[bad[:5]])
    return est, got


@pytest.mark.parametrize("s,r", [(0, 18), (2, 16)])
@pytest.mark.parametrize("n_hist", [3, 64, 8192])
def test_solve_equals_the_model_on_sketches_of_the_accuracy_input(lib, oracle, s, r, n_hist):
    w, h = M.accuracy_hashes(oracle)
    table, _ = M.add(*M.empty(r), w, h, s, r)
    check_against_model(lib, M.histogram(table, n_hist), s, r)


def test_solve_on_hand_made_histograms(lib):
    r = 10
    R = 1 << r
    # all counters empty: nothing was seen
    est, f = check_against_model(lib, [R] + [0] * 7, 3, r)
    assert est.distinct == 0.0 and est.occupancy == 0.0 and not f.any()
    # only t[0] and t[1]
    est, f = check_against_model(lib, [R - 100, 100, 0, 0], 0, r)
    assert 100 < est.distinct < 110 and est.singletons > 0
    # a non-zero overflow bin
    est, _ = check_against_model(lib, [R - 300, 200, 50, 30, 20], 1, r)
    assert est.overflow_buckets == 20
    # the smallest histogram, the largest table and sampling rate
    check_against_model(lib, [(1 << 28) - 7, 4, 3], 32, 28)


def test_solve_refuses_a_full_table_and_a_wrong_sum_and_writes_nothing(lib):
    from btl_bloomfilter_amd import _lib as L

    R = 1 << 8
    for t, word in (([0, R - 10, 10], b"full"), ([R - 10, 5, 4], b"histogram"), ([R, 1, 0], b"histogram"),
                    ([2**64 - 1, 2, R - 1], b"histogram")):
        rc, est, f = lib_solve(lib, t, 0, 8)
        assert rc == L.EINVAL and word in lib.btlbf_last_error(), (t, lib.btlbf_last_error())
        assert bytes(est) == b"\xa5" * C.sizeof(est) and f.tobytes() == b"\xa5" * f.nbytes
    rc, _, _ = lib_solve(lib, [0, R - 10, 10], 0, 8)
    assert b"table_bits" in lib.btlbf_last_error() and b"sample_bits" in lib.btlbf_last_error()


def test_accuracy_of_the_definition(oracle):
    w, h = M.accuracy_hashes(oracle)
    assert w == h.size == 4096 * 76
    distinct, once = M.accuracy_truth(oracle)
    table, totals = M.add(*M.empty(18), w, h, 0, 18)
    assert list(totals) == [w, w, w]
    F0, f, occ = M.solve(M.histogram(table, 64), 0, 18)
    print("s=0 r=18: distinct %d estimate %.1f (%+.2f %%); singletons %d estimate %.1f (%+.2f %%); occupancy %.3f"
          % (distinct, F0, 100 * (F0 / distinct - 1), once, f[1], 100 * (f[1] / once - 1), occ))
    assert abs(F0 / distinct - 1) <= 0.02
    assert abs(f[1] / once - 1) <= 0.03
    table, totals = M.add(*M.empty(16), w, h, 2, 16)
    F0, f, occ = M.solve(M.histogram(table, 64), 2, 16)
    print("s=2 r=16: distinct %d estimate %.1f (%+.2f %%); sampled %d of %d; occupancy %.3f"
          % (distinct, F0, 100 * (F0 / distinct - 1), totals[2], w, occ))
    assert abs(F0 / distinct - 1) <= 0.05


def test_library_exports_the_symbols_and_the_python_layer(lib):
    from btl_bloomfilter_amd import _lib as L
    import btl_bloomfilter_amd as m

    for name in ("create", "destroy", "clear", "add_seqs", "add_fastx", "merge", "download", "upload", "histogram", "solve",
                 "estimate_now"):
        assert hasattr(lib, "btlbf_card_" + name) and "btlbf_card_" + name in L.EXPORTS
    assert C.sizeof(L.CardEstimate) == 56
    assert callable(m.KmerCardinality) and callable(m.solve_spectrum)
    e = m.solve_spectrum([1 << 10] + [0] * 3, 0, 10)
    assert e.distinct == 0.0 and e.spectrum.size == 2 and e.at_least(1) == 0.0
    t = [1024 - 300, 200, 50, 30, 20]
    e = m.solve_spectrum(t, 1, 10)
    F0, f, occ = M.solve(t, 1, 10)
    assert close(e.distinct, F0, F0) and close(e.at_least(3), F0 - f[1] - f[2], F0) and e.overflow_buckets == 20
    with pytest.raises(ValueError):
        e.at_least(0)


def test_argument_errors_before_any_hip_call(lib, tmp_path):
    from btl_bloomfilter_amd import _lib as L

    h = C.c_void_p(99)
    for k, s, r, word in ((0, 11, 22, b"kmer_size"), (32769, 11, 22, b"kmer_size"), (25, 33, 22, b"sample_bits"),
                          (25, 11, 5, b"table_bits"), (25, 11, 29, b"table_bits")):
        assert lib.btlbf_card_create(C.byref(h), k, s, r, 0) == L.EINVAL and not h.value
        assert word in lib.btlbf_last_error(), lib.btlbf_last_error()
        h = C.c_void_p(99)
    assert lib.btlbf_card_create(None, 25, 11, 22, 0) == L.EINVAL
    seq = np.frombuffer(b"ACGT" * 10, np.uint8).copy()
    assert lib.btlbf_card_add_seqs(None, ptr(seq), 40, None, L.HOST, None) == L.EINVAL
    assert lib.btlbf_card_add_seqs(FAKE, None, 40, None, L.HOST, None) == L.EINVAL and b"null" in lib.btlbf_last_error()
    assert lib.btlbf_card_add_seqs(FAKE, ptr(seq), 40, None, 7, None) == L.EINVAL and b"mem" in lib.btlbf_last_error()
    lay = L.Layout(None, 0, 30)
    assert lib.btlbf_card_add_seqs(FAKE, ptr(seq), 40, C.byref(lay), L.HOST, None) == L.EINVAL
    assert b"read_len" in lib.btlbf_last_error()
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    assert lib.btlbf_card_add_fastx(None, str(fq).encode(), 0, 0, None) == L.EINVAL
    assert lib.btlbf_card_add_fastx(FAKE, None, 0, 0, None) == L.EINVAL
    assert lib.btlbf_card_add_fastx(FAKE, str(tmp_path / "missing.fq").encode(), 0, 0, None) == L.EIO
    assert b"missing.fq" in lib.btlbf_last_error()
    t = np.full(8, 7, np.uint64)
    f = np.full(8, 7.0)
    est = L.CardEstimate()
    for n_hist in (0, 2, 8193):
        assert lib.btlbf_card_histogram(FAKE, ptr(t), n_hist) == L.EINVAL and b"n_hist" in lib.btlbf_last_error()
        assert lib.btlbf_card_estimate_now(FAKE, n_hist, C.byref(est), ptr(f)) == L.EINVAL
        assert lib.btlbf_card_solve(ptr(t), n_hist, 0, 10, C.byref(est), ptr(f)) == L.EINVAL
    assert (t == 7).all() and (f == 7.0).all()
    assert lib.btlbf_card_solve(ptr(t), 8, 33, 10, C.byref(est), ptr(f)) == L.EINVAL
    assert lib.btlbf_card_solve(ptr(t), 8, 0, 29, C.byref(est), ptr(f)) == L.EINVAL
    for args in ((None, 8, 0, 10, C.byref(est), ptr(f)), (ptr(t), 8, 0, 10, None, ptr(f)), (ptr(t), 8, 0, 10, C.byref(est), None)):
        assert lib.btlbf_card_solve(*args) == L.EINVAL and b"null" in lib.btlbf_last_error()
    assert lib.btlbf_card_histogram(None, ptr(t), 8) == L.EINVAL and lib.btlbf_card_histogram(FAKE, None, 8) == L.EINVAL
    assert lib.btlbf_card_estimate_now(None, 8, C.byref(est), ptr(f)) == L.EINVAL
    assert lib.btlbf_card_estimate_now(FAKE, 8, None, ptr(f)) == L.EINVAL
    assert lib.btlbf_card_estimate_now(FAKE, 8, C.byref(est), None) == L.EINVAL
    tab = np.zeros(64, np.uint32)
    for fn in (lib.btlbf_card_download, lib.btlbf_card_upload):
        assert fn(None, ptr(tab), ptr(t)) == L.EINVAL and fn(FAKE, None, ptr(t)) == L.EINVAL
        assert fn(FAKE, ptr(tab), None) == L.EINVAL
    assert lib.btlbf_card_merge(None, FAKE) == L.EINVAL and lib.btlbf_card_merge(FAKE, None) == L.EINVAL
    assert lib.btlbf_card_merge(FAKE, FAKE) == L.EINVAL
    assert lib.btlbf_card_clear(None) == L.EINVAL
    lib.btlbf_card_destroy(None)


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_refusals_on_sketch_objects(tmp_path):
    """tests/cpp/test_card_refusals.cpp: the refusals on the library's own sketch object, built on the host"""
    exe = str(tmp_path / "test_card_refusals")
    libdir = os.path.join(ROOT, "btl_bloomfilter_amd")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function",
                        os.path.join(ROOT, "tests", "cpp", "test_card_refusals.cpp"), "-L" + libdir, "-lbtlbf",
                        "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    r = subprocess.run([exe, str(fq)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all cardinality refusals in place" in r.stdout, r.stdout + r.stderr


def test_cpp_layer_over_its_stub_abi(tmp_path):
    """btlbf::KmerCardinality (include/btlbf/KmerCardinality.hpp) over tests/cpp/stub_abi_card.cpp: what the class passes
    down and hands back, without the library; and the example compiles against the header"""
    exe = str(tmp_path / "test_card_shim")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_card_shim.cpp"),
           os.path.join(ROOT, "tests", "cpp", "stub_abi_card.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "card shim test passed" in r.stdout, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
