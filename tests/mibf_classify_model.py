"""Plain Python restatement of the reference's read classification, MIBFQuerySupport<T>::query(itr, minCount)
(MIBFQuerySupport.hpp:95-109, 398-428, 430-542, 555-595), over mibf_model.query: the checker of
tests/test_gpu_mibf_classify.py, pinned to the reference's own build by tests/test_mibf_classify_vs_ref.py.

Inputs are the hash rows of ONE sequence's emitted windows (its frames, in position order)."""
import math

import numpy as np

import mibf_model as mm

FIELDS = ("id", "count", "nonSatCount", "totalCount", "totalNonSatCount", "nonSatFrameCount", "solidCount")
_C, _NS, _T, _TNS, _NSF, _S = range(6)


def compare_std_err(a, b):
    """compareStdErr (:296-304)"""
    sa, sb = math.sqrt(a), math.sqrt(b)
    if a > b:
        return (float(a) - sa) <= (float(b) + sb)
    return (float(b) - sb) <= (float(a) + sa)


def compare_std_err_larger(a, b, extra_count):
    """compareStdErrLarger (:309-314); Python floats are IEEE doubles and nothing is fused"""
    sa = math.sqrt(a) * extra_count
    sb = math.sqrt(b) * extra_count
    return (float(a) - sa) <= (float(b) + sb)


def _u16(x):
    return x & 0xFFFF


def classify(data, ranks, rows, id_bytes, spaced, per_frame_prob, min_count_per_id, extra_count=1.0,
             extra_frame_limit=0, max_miss=0, min_count=1, best_hit_agree=False):
    """-> (results, satCount, evalCount); results = [(id, count, nonSatCount, totalCount, totalNonSatCount,
    nonSatFrameCount, solidCount)] in the reference's order"""
    mask, anti, _ = mm.masks(id_bytes)
    if len(rows) == 0:
        return [], 0, 0  # emptyResult
    rows = np.asarray(rows, np.uint64).reshape(len(rows), -1)
    n, h = rows.shape
    vals, match = mm.query(data, ranks, rows, np.ones(n, bool), max_miss, spaced)
    bit = ranks.bit(rows.ravel()).reshape(n, h)
    counts = {}  # id -> [count, nonSatCount, totalCount, totalNonSatCount, nonSatFrameCount, solidCount]
    cand = []
    best = [0] * 6
    second = 0
    sat_count = eval_count = extra_frame = 0

    def update_max(c):  # updateMaxCounts (:520-542)
        nonlocal second
        if c[_NSF] > best[_NSF]:
            best[_NSF] = c[_NSF]
        elif c[_NSF] > second:
            second = c[_NSF]
        for f in (_C, _NS, _S, _T, _TNS):
            if c[f] > best[f]:
                best[f] = c[f]

    for p in range(n):
        found = False
        if match[p]:
            # updatesCounts (:430-518)
            misses = int(h - bit[p].sum()) if spaced else 0
            seen = []
            fsat = 0
            for i in range(h):
                if not bit[p, i]:
                    continue
                raw = int(vals[p, i])
                eval_count += 1
                sat = raw > mask
                res = raw & anti if sat else raw
                c = counts.setdefault(res, [0] * 6)
                if sat:
                    fsat += 1
                else:
                    c[_TNS] = _u16(c[_TNS] + 1)
                c[_T] = _u16(c[_T] + 1)
                if raw not in seen:
                    if sat:
                        if res not in seen:
                            c[_C] = _u16(c[_C] + 1)
                    else:
                        c[_NS] = _u16(c[_NS] + 1)
                        c[_C] = _u16(c[_C] + 1)
                    seen.append(raw)
            if fsat == 0:
                for r in seen:
                    counts[r][_NSF] = _u16(counts[r][_NSF] + 1)
                    if misses == 0:
                        counts[r][_S] = _u16(counts[r][_S] + 1)
            else:
                sat_count += 1
            for r in seen:
                if r > mask:
                    if (r & anti) in seen:
                        continue
                    r &= anti
                c = counts[r]
                if c[_C] >= min_count_per_id[r]:
                    if r not in cand:
                        cand.append(r)
                    update_max(c)
                elif cand and c[_C] >= best[_C]:
                    if r not in cand:
                        cand.append(r)
                    update_max(c)
            if compare_std_err(best[_TNS], second):
                extra_frame = 0
            if best[_NSF] > second:
                old = extra_frame
                extra_frame += 1
                if extra_frame_limit < old:  # m_extraFrameLimit < extraFrame++
                    found = True
        if not spaced:
            eval_count += 1  # :415
        if found:
            break

    # summarizeCandiates (:555-595)
    out = []
    if cand and min_count <= best[_NSF]:
        signif = []
        for r in cand:
            c = counts[r]
            if (compare_std_err(best[_C], c[_C]) or compare_std_err(best[_TNS], c[_TNS]) or
                    compare_std_err(best[_NSF], c[_NSF]) or compare_std_err(best[_S], c[_S]) or
                    compare_std_err(best[_NS], c[_NS]) or compare_std_err(best[_T], c[_T])):  # isValid (:333-342)
                signif.append((r,) + tuple(c))
        if len(signif) > 1:
            # sortCandidates (:230-246); Python's sort is stable: full ties keep the candidate-list order
            signif.sort(key=lambda q: (-q[1 + _NSF], -q[1 + _C], -q[1 + _S], -q[1 + _NS], -q[1 + _TNS], -q[1 + _T],
                                       -per_frame_prob[q[0]]))
            a = signif[0]
            for q in signif:
                if all(compare_std_err_larger(a[1 + f], q[1 + f], extra_count) for f in (_C, _TNS, _NSF, _S, _NS, _T)):
                    out.append(q)
            if best_hit_agree and len(out) >= 2:
                b, a2 = out[0], out[1]
                if not all(b[1 + f] >= a2[1 + f] for f in range(6)):  # checkCountAgreement (:358-364)
                    out = []
        elif signif:
            out = [signif[0]]
    return out, sat_count, eval_count
