"""numpy restatement of the read screen's verdict and tally (include/btlbf.h: btlbf_screen_seqs' pass_bits,
btlbf_screen_tally), what the GPU results are compared with.  No test of its own."""
import numpy as np


def verdict_model(hits, valid, min_fraction, min_hits):
    """pass_bits[n]: bit j = valid > 0 and hits[:, j] >= min_hits and float64(hits[:, j]) >= min_fraction * float64(valid)
    -- one IEEE double multiply and one compare, as the header states it"""
    hits = np.asarray(hits).astype(np.uint32)
    valid = np.asarray(valid).astype(np.uint32)
    need = np.float64(min_fraction) * valid.astype(np.float64)
    ok = (valid[:, None] > 0) & (hits >= np.uint32(min_hits)) & (hits.astype(np.float64) >= need[:, None])
    return (ok.astype(np.uint32) << np.arange(hits.shape[1], dtype=np.uint32)).sum(axis=1).astype(np.uint32)


def tally_model(hits, valid, pass_bits):
    """(passed[F], best[F], totals[4]) of the rows: rows passing filter j; rows whose passing filter with the most hits
    is j, ties to the lowest j; {rows, rows passing none, rows passing two or more, rows with valid == 0}"""
    hits = np.asarray(hits).astype(np.int64)
    valid = np.asarray(valid)
    nf = hits.shape[1]
    ok = ((np.asarray(pass_bits).astype(np.uint32)[:, None] >> np.arange(nf, dtype=np.uint32)) & 1).astype(bool)
    passed = ok.sum(axis=0).astype(np.uint64)
    score = np.where(ok, hits, -1)
    any_ = ok.any(axis=1)
    best = np.bincount(score.argmax(axis=1)[any_], minlength=nf).astype(np.uint64)  # argmax: the first of equal maxima
    n_ok = ok.sum(axis=1)
    totals = np.array([len(valid), (n_ok == 0).sum(), (n_ok >= 2).sum(), (valid == 0).sum()], np.uint64)
    return passed, best, totals
