"""The filter algebra (btlbf_clone / btlbf_combine / btlbf_fold / btlbf_threshold_bits) without a GPU: the symbols and
constants in the library, the Python table and the header; the argument errors that are reported before a filter is looked
at; every refusal that looks at the filters, on the library's own filter objects built on the host by
tests/cpp/test_algebra_refusals.cpp (a handle cannot be made without a GPU); and the C++ layer compiling against the
headers."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW = ["btlbf_clone", "btlbf_combine", "btlbf_fold", "btlbf_threshold_bits"]


def test_library_exports_the_symbols(lib):
    from btl_bloomfilter_amd import _lib

    text = open(os.path.join(ROOT, "include", "btlbf.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTS and re.search(r"\bint %s\(" % name, text), name
    names = ["OR", "AND", "ANDNOT", "ADD", "MAX", "MIN"]
    for value, name in enumerate(names):
        assert getattr(_lib, "COMBINE_" + name) == value and "BTLBF_COMBINE_%s = %d" % (name, value) in text
    assert _lib.COMBINE_MAX_SRCS == 16 and "#define BTLBF_COMBINE_MAX_SRCS 16" in text
    import btl_bloomfilter_amd as m

    for cls, members in ((m.BloomFilter, ["copy", "combine", "fold", "union", "intersect", "subtract", "__or__", "__iand__"]),
                         (m.CountingBloomFilter, ["copy", "combine", "fold", "merge", "toBloomFilter"])):
        for name in members:
            assert callable(getattr(cls, name)), name


def test_argument_errors_before_any_filter_is_looked_at(lib):
    from btl_bloomfilter_amd import _lib as L

    FAKE = 16  # never dereferenced
    pop = C.c_uint64(7)
    two = (C.c_void_p * 2)(FAKE + 16, FAKE + 32)
    for args, word in (((None, two, 2, L.COMBINE_OR), b"null"), ((FAKE, None, 2, L.COMBINE_OR), b"null"),
                       ((FAKE, two, 0, L.COMBINE_OR), b"n_srcs"), ((FAKE, two, 17, L.COMBINE_OR), b"n_srcs"),
                       ((FAKE, (C.c_void_p * 2)(FAKE + 16, None), 2, L.COMBINE_OR), b"null handle"),
                       ((FAKE, (C.c_void_p * 2)(FAKE + 16, FAKE), 2, L.COMBINE_OR), b"among the sources")):
        assert lib.btlbf_combine(*args, C.byref(pop)) == L.EINVAL and word in lib.btlbf_last_error(), word
        assert pop.value == 7
    for call in (lambda out: lib.btlbf_clone(out, None), lambda out: lib.btlbf_fold(out, None, 2),
                 lambda out: lib.btlbf_threshold_bits(out, None, 1)):
        h = C.c_void_p(99)
        assert call(C.byref(h)) == L.EINVAL and b"null" in lib.btlbf_last_error() and not h.value
    assert lib.btlbf_clone(None, FAKE) == L.EINVAL and lib.btlbf_fold(None, FAKE, 2) == L.EINVAL
    assert lib.btlbf_threshold_bits(None, FAKE, 1) == L.EINVAL


def test_refusals_on_filter_objects(tmp_path):
    exe = str(tmp_path / "test_algebra_refusals")
    libdir = os.path.join(ROOT, "btl_bloomfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function",
                        os.path.join(ROOT, "tests", "cpp", "test_algebra_refusals.cpp"), "-L" + libdir, "-lbtlbf",
                        "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all algebra refusals in place" in r.stdout, r.stdout + r.stderr


def test_cpp_layer_compiles_on_cpu(tmp_path):
    from test_gpu_cpp_screen import build_program

    assert os.path.exists(build_program(tmp_path, os.path.join("examples", "bloom_merge.cpp")))
    assert os.path.exists(build_program(tmp_path, os.path.join("tests", "cpp", "test_algebra_shim.cpp")))
