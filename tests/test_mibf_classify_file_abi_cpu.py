"""The file classifier, the frame probabilities and the two device helpers without a GPU: the symbols, every argument
error that is reported before any HIP call (with a handle that is never dereferenced, and outputs untouched), and the C++
layer's members compiling against the header."""
import ctypes as C
import os

import numpy as np

from test_gpu_cpp_mibf_classify_file import build_program

FAKE = C.c_void_p(16)  # never dereferenced: every call below fails before it looks at the miBF
NEW = ["btlbf_mibf_frame_probs", "btlbf_mibf_prob_single_frame", "btlbf_interleave_mates", "btlbf_mibf_classify_tally",
       "btlbf_mibf_classify_fastx_open", "btlbf_mibf_classify_fastx_next", "btlbf_mibf_classify_fastx_tally",
       "btlbf_mibf_classify_fastx_close", "btlbf_mibf_classify_fastx"]
ptr = lambda a: C.c_void_p(a.ctypes.data)


def test_library_exports_the_symbols(lib):
    from btl_bloomfilter_amd import _lib

    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.FASTX_WHOLE == 4 and _lib.CLASSIFY_INTERLEAVED == 256


def test_prob_single_frame_needs_no_device(lib):
    from mibf_frame_probs_model import prob_single_frame

    for args in [(0.3, 4, 0.1, 0), (0.3, 4, 0.1, 1), (0.25, 1, 1.0 / 1024, 0), (0.5, 8, 0.01, 8), (0.3, 4, 0.0, 2)]:
        assert lib.btlbf_mibf_prob_single_frame(*args) == prob_single_frame(*args), args
    assert lib.btlbf_mibf_prob_single_frame(0.3, 4, 0.1, 5) == 0.0  # the reference's wrapped loop does not run


def test_frame_probs_argument_errors(lib):
    from btl_bloomfilter_amd import _lib as L

    probs = np.full(4, -7.5)
    sat = C.c_double(-1.0)
    for m, p, n, s in [(None, ptr(probs), 4, C.byref(sat)), (FAKE, None, 4, C.byref(sat)), (FAKE, ptr(probs), 4, None),
                       (FAKE, ptr(probs), 0, C.byref(sat))]:
        assert lib.btlbf_mibf_frame_probs(m, 0, p, n, s) == L.EINVAL
        assert (probs == -7.5).all() and sat.value == -1.0


def test_helper_argument_errors(lib):
    from btl_bloomfilter_amd import _lib as L

    seq = np.frombuffer(b"ACGT" * 4, np.uint8).copy()
    st = np.array([0, 8, 16], np.uint64)
    out, out_st = np.full(32, 7, np.uint8), np.full(5, 7, np.uint64)
    for null in (1, 3, 6):
        args = [ptr(seq), ptr(st), ptr(seq), ptr(st), 2, ptr(out), ptr(out_st), L.HOST, 0, None]
        args[null] = None
        assert lib.btlbf_interleave_mates(*args) == L.EINVAL and b"null" in lib.btlbf_last_error()
        assert (out == 7).all() and (out_st == 7).all()
    hits, three = np.zeros((2, 2, 4), np.uint32), [np.zeros(2, np.uint32) for _ in range(3)]
    tot = [np.full(4, 7, np.uint64), np.full(4, 7, np.uint64), np.full(6, 7, np.uint64)]

    def tally(null=None, max_results=2, n_ids=4):
        args = [ptr(hits)] + [ptr(x) for x in three] + [2, max_results, n_ids] + [ptr(x) for x in tot] + [L.HOST, 0, None]
        if null is not None:
            args[null] = None
        rc = lib.btlbf_mibf_classify_tally(*args)
        assert all((x == 7).all() for x in tot)
        return rc

    for null in (0, 1, 2, 3, 7, 8, 9):
        assert tally(null=null) == L.EINVAL and b"null" in lib.btlbf_last_error(), null
    assert tally(max_results=0) == L.EINVAL and tally(n_ids=0) == L.EINVAL


def test_file_classifier_argument_errors(lib, tmp_path):
    from btl_bloomfilter_amd import _lib as L

    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    path, missing = str(fq).encode(), str(tmp_path / "missing.fq").encode()
    prob, minc = np.zeros(4, np.float64), np.ones(4, np.uint32)
    tot = [np.full(4, 7, np.uint64), np.full(4, 7, np.uint64), np.full(6, 7, np.uint64)]

    def open_(m=FAKE, p1=path, p2=None, flags=0, max_results=2, n_ids=4, null=None):
        h = C.c_void_p(99)
        par = L.MibfClassifyParams(1.0, 0, 0, 1, 0, max_results)
        args = [C.byref(h), m, p1, p2, flags, C.byref(par), ptr(prob), ptr(minc), n_ids, 0]
        if null is not None:
            args[null] = None
        rc = lib.btlbf_mibf_classify_fastx_open(*args)
        assert rc != 0 and h.value in (None, 99)  # no handle comes back
        whole = [m, p1, p2, flags, C.byref(par), ptr(prob), ptr(minc), n_ids, 0] + [ptr(x) for x in tot] + [None]
        if null == 0:  # the handle pointer: the whole-file call has none
            return rc
        if null is not None:
            whole[null - 1] = None
        assert lib.btlbf_mibf_classify_fastx(*whole) == rc and all((x == 7).all() for x in tot)
        return rc

    assert open_(m=None) == L.EINVAL
    for null in (0, 2, 5, 6, 7):
        assert open_(null=null) == L.EINVAL and b"null" in lib.btlbf_last_error(), null
    assert open_(max_results=0) == L.EINVAL and b"max_results" in lib.btlbf_last_error()
    assert open_(n_ids=0) == L.EINVAL and b"n_ids" in lib.btlbf_last_error()
    assert open_(p2=path, flags=L.CLASSIFY_INTERLEAVED) == L.EINVAL and b"not both" in lib.btlbf_last_error()
    assert open_(p1=missing) == L.EIO and open_(p2=missing) == L.EIO and b"missing.fq" in lib.btlbf_last_error()
    n = C.c_uint64(7)
    assert lib.btlbf_mibf_classify_fastx_next(None, C.byref(n), C.byref(n), None, None, None, None) == L.EINVAL
    assert lib.btlbf_mibf_classify_fastx_tally(None, ptr(tot[0]), ptr(tot[1]), ptr(tot[2])) == L.EINVAL
    lib.btlbf_mibf_classify_fastx_close(None)
    for i in range(3):  # the whole-file call's own outputs
        args = [FAKE, path, None, 0, C.byref(L.MibfClassifyParams(1.0, 0, 0, 1, 0, 2)), ptr(prob), ptr(minc), 4, 0] + \
            [ptr(x) for x in tot] + [None]
        args[9 + i] = None
        assert lib.btlbf_mibf_classify_fastx(*args) == L.EINVAL


def test_cpp_members_compile_on_cpu(tmp_path):
    assert os.path.exists(build_program(tmp_path, os.path.join("examples", "mibf_classify.cpp")))
    assert os.path.exists(build_program(tmp_path, os.path.join("tests", "cpp", "test_mibf_file_shim.cpp")))
