"""btlbf_mibf_classify_tally restated in numpy: the summary of classify results (include/btlbf.h)."""
import numpy as np


def tally_model(hits, n_hits, sat_count, eval_count, n_ids, max_results=None):
    """hits: [n_rows, max_results] records with an "id" field (HIT_DTYPE) -> (best[n_ids], any[n_ids], totals[6])"""
    n_hits = np.asarray(n_hits, np.uint32)
    max_results = hits.shape[1] if max_results is None else max_results
    best, any_ = np.zeros(n_ids, np.uint64), np.zeros(n_ids, np.uint64)
    for r, nh in enumerate(n_hits):
        for j in range(min(int(nh), max_results)):
            i = int(hits[r, j]["id"])
            if i < n_ids:
                any_[i] += 1
                if j == 0:
                    best[i] += 1
    totals = np.array([len(n_hits), (n_hits == 0).sum(), (n_hits > 1).sum(), (n_hits > max_results).sum(),
                       np.asarray(sat_count, np.uint64).sum(), np.asarray(eval_count, np.uint64).sum()], np.uint64)
    return best, any_, totals
