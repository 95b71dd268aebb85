"""The paired calls of btlbf::MIBFQuerySupport<T> (include/btlbf/MIBFQuerySupport.hpp) over btlbf_mibf_classify_pairs:
tests/cpp/test_mibf_pair_query_shim.cpp builds a miBF through the C++ layer, classifies the pairs of
tests/test_mibf_classify_pairs_vs_ref.py through query(seq1, seq2, minCount) and through queryPairs, and its output must
equal the model that test pins to the reference.  (That the program compiles without a GPU is checked by
tests/test_mibf_classify_pairs_abi_cpu.py.)"""
import os
import subprocess

import pytest

import test_mibf_classify_pairs_vs_ref as pr
import test_mibf_classify_vs_ref as cr
from conftest import ROOT


def build_program(tmp_path):
    from btl_bloomfilter_amd import build

    build.build()
    exe = str(tmp_path / "test_mibf_pair_query_shim")
    lib_dir = os.path.join(ROOT, "btl_bloomfilter_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "test_mibf_pair_query_shim.cpp"), "-L" + lib_dir, "-lbtlbf",
                        "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,id_bytes", [("C5", 2), ("nt3", 4)])
def test_pair_query_shim_against_pinned_model(oracle, tmp_path, monkeypatch, cfg, id_bytes):
    exe = build_program(tmp_path)
    seeds, h = cr.CFGS[cfg]
    _, _, entries, occ, _, _, _ = cr.make_case(cfg, id_bytes)
    size = cr.optimal_size(entries, h, occ)
    ps = cr.param_sets(bool(seeds))[::5]
    monkeypatch.setattr(cr, "param_sets", lambda spaced: ps)
    got_size, data, res = pr.run_pair_driver(exe, tmp_path, monkeypatch, cfg, id_bytes)
    monkeypatch.undo()
    ranks, model_data = cr.build_model_mibf(oracle, cfg, id_bytes, size)
    assert got_size == size and (data == model_data).all()
    for pi, p in enumerate(ps):
        exp = pr.model_pairs(oracle, cfg, id_bytes, ranks, model_data, p)
        assert len(exp) == 20
        for qi, e in enumerate(exp):
            recs, sat, ev, _ = res[pi, qi]
            assert [[list(r) for r in recs], sat, ev] == e, (p, qi)
