"""btlbf_mibf_classify_pairs without a GPU: the symbol, the argument errors reported before any HIP call (and before
the handle is looked at), and the C++ layer's paired calls compiling against the header."""
import ctypes as C
import os

import numpy as np

from test_gpu_cpp_mibf_pair_query import build_program

FAKE = C.c_void_p(16)  # never dereferenced: every call below fails before it looks at the miBF


def test_library_exports_the_symbol(lib):
    from btl_bloomfilter_amd import _lib

    assert hasattr(lib, "btlbf_mibf_classify_pairs")
    assert "btlbf_mibf_classify_pairs" in _lib.EXPORTS
    assert lib.btlbf_mibf_classify_pairs.argtypes == lib.btlbf_mibf_classify_seqs.argtypes


def test_argument_errors_come_before_any_hip_call(lib):
    from btl_bloomfilter_amd import _lib as L

    seq = np.frombuffer(b"ACGT" * 40, np.uint8).copy()
    even = np.array([0, 40, 80, 120, 160], np.uint64)
    odd = np.array([0, 40, 80, 160], np.uint64)
    prob, minc = np.zeros(4, np.float64), np.ones(4, np.uint32)
    hits = np.full((2, 2, 4), 0xABABABAB, np.uint32)
    outs = [np.full(2, 7, np.uint32) for _ in range(3)]
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def call(m=FAKE, starts=even, n_seqs=4, read_len=0, max_results=2, n_ids=4, null=None):
        lay = L.Layout(ptr(starts) if starts is not None else None, n_seqs, read_len)
        par = L.MibfClassifyParams(1.0, 0, 0, 1, 0, max_results)
        args = [m, ptr(seq), seq.size, C.byref(lay), C.byref(par), ptr(prob), ptr(minc), n_ids, ptr(hits), ptr(outs[0]),
                ptr(outs[1]), ptr(outs[2]), L.HOST, None]
        if null is not None:
            args[null] = None
        rc = lib.btlbf_mibf_classify_pairs(*args)
        assert (hits == 0xABABABAB).all() and all((o == 7).all() for o in outs)
        return rc

    assert call(m=None) == L.EINVAL
    for null in (1, 3, 4, 5, 6, 8, 9, 10, 11):
        assert call(null=null) == L.EINVAL, null
        assert b"null" in lib.btlbf_last_error()
    assert call(max_results=0) == L.EINVAL and b"max_results" in lib.btlbf_last_error()
    assert call(n_ids=0) == L.EINVAL and b"n_ids" in lib.btlbf_last_error()
    assert call(starts=odd, n_seqs=3) == L.EINVAL and b"even" in lib.btlbf_last_error()
    assert call(starts=None, n_seqs=0, read_len=32) == L.EINVAL and b"even" in lib.btlbf_last_error()  # 160 / 32 = 5


def test_pair_query_shim_compiles_on_cpu(tmp_path):
    assert os.path.exists(build_program(tmp_path))
