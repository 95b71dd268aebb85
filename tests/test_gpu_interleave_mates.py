"""btlbf_interleave_mates (interleave_mates_device) against the host function interleave_mates, byte for byte and
offset for offset: pair counts 0, 1 and 65 (one wavefront per pair: several workgroups of four),
mates of 0, 1, 63, 64, 65 and 300 bases (none, one lane, one short of / exactly / one over a wavefront's 64 bytes,
several rounds), both inputs at odd base offsets."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mibf_classify import bf  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
LENS = [0, 1, 63, 64, 65, 300]


def mates(n_pairs, seed):
    rng = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGTN", np.uint8)
    pick = lambda i: acgt[rng.randint(0, 5, LENS[i % len(LENS)])]
    # every length meets every length once n_pairs >= 36: mate 1 cycles through LENS, mate 2 a step slower
    return [pick(i) for i in range(n_pairs)], [pick(i // len(LENS) + i) for i in range(n_pairs)]


def ragged(reads):
    starts = np.zeros(len(reads) + 1, np.int64)
    if reads:
        starts[1:] = np.cumsum([r.size for r in reads])
    return (np.concatenate(reads) if reads else np.zeros(0, np.uint8)), starts


@pytest.mark.parametrize("n_pairs", [0, 1, 65])
def test_device_equals_host(bf, n_pairs):  # noqa: F811
    import torch

    r1, r2 = mates(n_pairs, n_pairs)
    if n_pairs == 65:
        assert {(a.size, b.size) for a, b in zip(r1, r2)} >= {(x, y) for x in LENS for y in LENS}
    if n_pairs == 1:
        r1, r2 = [r1[0][:0]], [np.frombuffer(b"ACGTT", np.uint8)]  # an empty first mate
    exp_seq, exp_starts = bf.interleave_mates(r1, r2)
    (s1, st1), (s2, st2) = ragged(r1), ragged(r2)
    # the inputs at odd base offsets: slices at +1 and +3 of larger tensors
    big1 = torch.from_numpy(np.concatenate([[255], s1, [255]]).astype(np.uint8)).cuda()
    big2 = torch.from_numpy(np.concatenate([[254] * 3, s2, [254]]).astype(np.uint8)).cuda()
    d1, d2 = big1[1:1 + s1.size], big2[3:3 + s2.size]
    assert (not s1.size or d1.data_ptr() % 2 == 1) and (not s2.size or d2.data_ptr() % 2 == 1)
    out, out_starts = bf.interleave_mates_device(d1, torch.from_numpy(st1).cuda(), d2, torch.from_numpy(st2).cuda())
    torch.cuda.synchronize()
    assert out_starts.cpu().numpy().astype(np.uint64).tolist() == exp_starts.tolist()
    assert out.cpu().numpy().tobytes() == exp_seq.tobytes()
    # host memory through the same entry point
    o = np.full(max(exp_seq.size, 1), 7, np.uint8)
    os_ = np.full(2 * n_pairs + 1, 7, np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    s1c, s2c, st1u, st2u = np.ascontiguousarray(s1), np.ascontiguousarray(s2), st1.astype(np.uint64), st2.astype(np.uint64)
    rc = bf._lib.load().btlbf_interleave_mates(ptr(s1c), ptr(st1u), ptr(s2c), ptr(st2u), n_pairs, ptr(o), ptr(os_),
                                               bf._lib.HOST, 0, None)
    assert rc == 0 and os_.tolist() == exp_starts.tolist() and o[:exp_seq.size].tobytes() == exp_seq.tobytes()
