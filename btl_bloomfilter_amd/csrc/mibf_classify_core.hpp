// csrc/mibf_classify_core.hpp -- the device code the two classification walks share (mibf_classify_kernels.hip: one
// sequence; mibf_classify_pair_kernels.hip: the two mates of a pair, alternating): the slot table of m_counts, the loading
// of 64 windows, updatesCounts (MIBFQuerySupport.hpp:430-518) of one hit frame on the best / second-best state,
// summarizeCandiates (:555-595) and the result record.  Every lane of a wavefront runs these on the same values.
#pragma once
#include "internal.hpp"

namespace btlbf {

static constexpr uint32_t kClsEmpty = 0xffffffffu;
static constexpr uint32_t kClsWaves = 4; // tables (wavefronts) per workgroup of the LDS kernels
// a slot: {id, count | nonSatCount << 16, totalCount | totalNonSatCount << 16, nonSatFrameCount | solidCount << 16,
// 1 + position in the candidate list (0: no candidate), slot of candidate number <this slot's index>}
static constexpr uint32_t kSlotWords = kMibfClsSlotWords;

template <class T>
struct ClsMask {
	static constexpr uint32_t mask = 1u << (sizeof(T) * 8 - 1);
	static constexpr uint32_t anti = mask - 1;
};

// the reference's doubles: no fused multiply-add may stand in for a product and a sum
#pragma clang fp contract(off)

// compareStdErr (MIBFQuerySupport.hpp:296-304)
__device__ __forceinline__ bool cls_stderr(uint32_t a, uint32_t b)
{
	const double sa = __builtin_sqrt((double)a), sb = __builtin_sqrt((double)b);
	if (a > b)
		return ((double)a - sa) <= ((double)b + sb);
	return ((double)b - sb) <= ((double)a + sa);
}

// compareStdErrLarger (:309-314)
__device__ __forceinline__ bool cls_stderr_larger(uint32_t a, uint32_t b, double extra)
{
	const double sa = __builtin_sqrt((double)a) * extra, sb = __builtin_sqrt((double)b) * extra;
	return ((double)a - sa) <= ((double)b + sb);
}

struct ClsCounts { // CountResult / QueryResult, widened
	uint32_t count, nonSat, total, totalNonSat, nsFrame, solid;
};

__device__ __forceinline__ ClsCounts cls_load(const uint32_t* tab, uint32_t slot)
{
	const uint32_t w1 = tab[slot * kSlotWords + 1], w2 = tab[slot * kSlotWords + 2], w3 = tab[slot * kSlotWords + 3];
	return ClsCounts{w1 & 0xffffu, w1 >> 16, w2 & 0xffffu, w2 >> 16, w3 & 0xffffu, w3 >> 16};
}

// ++ of the uint16_t in the low / high half of a word, each wrapping on its own
__device__ __forceinline__ uint32_t inc_lo(uint32_t w) { return (w & 0xffff0000u) | ((w + 1) & 0xffffu); }
__device__ __forceinline__ uint32_t inc_hi(uint32_t w) { return w + 0x10000u; }

// the slot of `id`, claimed and zeroed (m_counts[id] = {0,...}, :447-453) when the walk meets the id for the first time.
// cap is a power of two above the number of distinct ids a walk can meet, so an empty slot always exists.
__device__ __forceinline__ uint32_t cls_slot(uint32_t* tab, uint32_t cap, uint32_t id)
{
	uint32_t s = ((id * 0x9E3779B1u) >> 7) & (cap - 1);
	for (;;) {
		const uint32_t key = tab[s * kSlotWords];
		if (key == id)
			return s;
		if (key == kClsEmpty) {
			tab[s * kSlotWords] = id;
			tab[s * kSlotWords + 1] = 0;
			tab[s * kSlotWords + 2] = 0;
			tab[s * kSlotWords + 3] = 0;
			tab[s * kSlotWords + 4] = 0;
			return s;
		}
		s = (s + 1) & (cap - 1);
	}
}

// sortCandidates (:230-246): does x come before y
__device__ __forceinline__ bool cls_before(const ClsCounts& x, double px, const ClsCounts& y, double py)
{
	if (x.nsFrame != y.nsFrame)
		return x.nsFrame > y.nsFrame;
	if (x.count != y.count)
		return x.count > y.count;
	if (x.solid != y.solid)
		return x.solid > y.solid;
	if (x.nonSat != y.nonSat)
		return x.nonSat > y.nonSat;
	if (x.totalNonSat != y.totalNonSat)
		return x.totalNonSat > y.totalNonSat;
	if (x.total != y.total)
		return x.total > y.total;
	return px > py;
}

// frame window: the frames of a sequence over [b, e) are its clean windows in position order; a walk takes them in
// chunks of 64 window starts, chunk c beginning here
__device__ __forceinline__ uint64_t cls_chunk_window(uint64_t b, uint64_t c) { return b + c * 64; }

template <class T>
__device__ __forceinline__ void cls_write_hit(const MibfClassifyArgs& a, uint64_t row, uint32_t at, uint32_t id,
                                              const ClsCounts& c)
{
	uint32_t* o = reinterpret_cast<uint32_t*>(a.hits) + (row * a.max_results + at) * 4;
	o[0] = id;
	o[1] = c.count | c.nonSat << 16;
	o[2] = c.total | c.totalNonSat << 16;
	o[3] = c.nsFrame | c.solid << 16;
}

// the 64 windows from gp0 on, window gp0 + lane in this lane: its raw values and hit mask (zero unless it matched);
// todo = the clean windows (the frames), mbits = those that hit.  Windows from e on are not read.
template <class T>
__device__ __forceinline__ void cls_load_chunk(const MibfClassifyArgs& a, uint64_t gp0, uint64_t e,
                                               uint32_t (&v)[kMibfMaxHash], uint32_t& hm, uint64_t& todo, uint64_t& mbits)
{
	const uint64_t gp = gp0 + (threadIdx.x & 63u);
	const T* values = static_cast<const T*>(a.values);
	bool ok = false, match = false;
	hm = 0;
#pragma unroll
	for (uint32_t i = 0; i < kMibfMaxHash; ++i)
		v[i] = 0;
	if (gp < e) {
		ok = (a.valid_bits[gp >> 6] >> (gp & 63)) & 1;
		match = (a.match_bits[gp >> 6] >> (gp & 63)) & 1;
		if (match) {
			hm = a.spaced ? a.hit_masks[gp] : (1u << a.h) - 1;
#pragma unroll
			for (uint32_t i = 0; i < kMibfMaxHash; ++i)
				if (i < a.h)
					v[i] = values[gp * a.h + i];
		}
	}
	todo = __ballot(ok);
	mbits = __ballot(match);
}

// what a walk carries from frame to frame (m_candidateMatches as n_cand entries of the table's word 5, the maxima of
// updateMaxCounts, m_satCount, m_evalCount, the extra frames of the early stop)
struct ClsState {
	uint32_t n_cand = 0, sat_count = 0, eval = 0, extra = 0;
	uint32_t b_count = 0, b_nonsat = 0, b_total = 0, b_totalns = 0, b_nsf = 0, b_solid = 0, second = 0;
	bool found = false;
};

// updatesCounts (:430-518) of one frame that hit: `hits` = its hit mask, fv = its raw values.  Sets st.found when the
// walk stops here (:102-105).
template <class T>
__device__ __forceinline__ void cls_frame(const MibfClassifyArgs& a, uint32_t* tab, uint32_t cap, ClsState& st,
                                          uint32_t hits, const uint32_t (&fv)[kMibfMaxHash])
{
	constexpr uint32_t mask = ClsMask<T>::mask, anti = ClsMask<T>::anti;
	const uint32_t h = a.h;
	const uint32_t misses = h - __popc(hits);
	uint32_t fslot[kMibfMaxHash];
#pragma unroll
	for (uint32_t i = 0; i < kMibfMaxHash; ++i)
		fslot[i] = 0;
	uint32_t seen = 0, fsat = 0; // seen: bit i = position i pushed its raw value onto m_seenSet
#pragma unroll
	for (uint32_t i = 0; i < kMibfMaxHash; ++i) {
		if (i >= h || !((hits >> i) & 1))
			continue;
		const uint32_t raw = fv[i];
		++st.eval;
		const bool sat = raw > mask;
		const uint32_t id = sat ? raw & anti : raw;
		fsat += sat;
		const uint32_t s = cls_slot(tab, cap, id);
		fslot[i] = s;
		uint32_t w2 = inc_lo(tab[s * kSlotWords + 2]);
		if (!sat)
			w2 = inc_hi(w2);
		tab[s * kSlotWords + 2] = w2;
		bool raw_seen = false, id_seen = false;
#pragma unroll
		for (uint32_t j = 0; j < kMibfMaxHash; ++j) {
			if (j < i && ((seen >> j) & 1)) {
				raw_seen |= fv[j] == raw;
				id_seen |= fv[j] == id;
			}
		}
		if (!raw_seen) {
			uint32_t w1 = tab[s * kSlotWords + 1];
			if (sat) {
				if (!id_seen)
					w1 = inc_lo(w1);
			} else {
				w1 = inc_lo(inc_hi(w1));
			}
			tab[s * kSlotWords + 1] = w1;
			seen |= 1u << i;
		}
	}
	if (fsat == 0) {
#pragma unroll
		for (uint32_t i = 0; i < kMibfMaxHash; ++i) {
			if (!((seen >> i) & 1))
				continue;
			uint32_t w3 = inc_lo(tab[fslot[i] * kSlotWords + 3]);
			if (misses == 0)
				w3 = inc_hi(w3);
			tab[fslot[i] * kSlotWords + 3] = w3;
		}
	} else {
		++st.sat_count;
	}
#pragma unroll
	for (uint32_t i = 0; i < kMibfMaxHash; ++i) {
		if (!((seen >> i) & 1))
			continue;
		const uint32_t raw = fv[i];
		if (raw > mask) {
			bool plain = false; // the non-saturated version is in the set too
#pragma unroll
			for (uint32_t j = 0; j < kMibfMaxHash; ++j)
				plain |= j != i && ((seen >> j) & 1) && fv[j] == (raw & anti);
			if (plain)
				continue;
		}
		const uint32_t s = fslot[i];
		const uint32_t id = tab[s * kSlotWords];
		const ClsCounts cr = cls_load(tab, s);
		if (cr.count >= a.min_count_per_id[id] || (st.n_cand && cr.count >= st.b_count)) {
			if (tab[s * kSlotWords + 4] == 0) {
				tab[st.n_cand * kSlotWords + 5] = s;
				tab[s * kSlotWords + 4] = ++st.n_cand;
			}
			// updateMaxCounts (:520-542)
			if (cr.nsFrame > st.b_nsf)
				st.b_nsf = cr.nsFrame;
			else if (cr.nsFrame > st.second)
				st.second = cr.nsFrame;
			st.b_count = cr.count > st.b_count ? cr.count : st.b_count;
			st.b_nonsat = cr.nonSat > st.b_nonsat ? cr.nonSat : st.b_nonsat;
			st.b_solid = cr.solid > st.b_solid ? cr.solid : st.b_solid;
			st.b_total = cr.total > st.b_total ? cr.total : st.b_total;
			st.b_totalns = cr.totalNonSat > st.b_totalns ? cr.totalNonSat : st.b_totalns;
		}
	}
	if (cls_stderr(st.b_totalns, st.second))
		st.extra = 0;
	if (st.b_nsf > st.second) {
		if (a.extra_frame_limit < st.extra++)
			st.found = true;
	}
}

// summarizeCandiates (:555-595) at the end of a walk, and its three counts; lane 0 writes result row `row`
template <class T>
__device__ __forceinline__ void cls_summarize(const MibfClassifyArgs& a, uint32_t* tab, const ClsState& st, uint64_t row)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t n_cand = st.n_cand, b_count = st.b_count, b_nonsat = st.b_nonsat, b_total = st.b_total,
	               b_totalns = st.b_totalns, b_nsf = st.b_nsf, b_solid = st.b_solid;
	uint32_t n_res = 0;
	if (n_cand && a.min_count <= b_nsf) {
		uint32_t nv = 0;
		for (uint32_t c = 0; c < n_cand; ++c) {
			const uint32_t s = tab[c * kSlotWords + 5];
			const ClsCounts r = cls_load(tab, s);
			// isValid (:333-342)
			if (cls_stderr(b_count, r.count) || cls_stderr(b_totalns, r.totalNonSat) || cls_stderr(b_nsf, r.nsFrame) ||
			    cls_stderr(b_solid, r.solid) || cls_stderr(b_nonsat, r.nonSat) || cls_stderr(b_total, r.total)) {
				tab[nv * kSlotWords + 5] = s;
				++nv;
			}
		}
		if (nv > 1) {
			// sort(signifResults, sortCandidates) as an insertion sort: full ties keep the candidate-list order
			for (uint32_t i = 1; i < nv; ++i) {
				const uint32_t s = tab[i * kSlotWords + 5];
				const ClsCounts x = cls_load(tab, s);
				const double px = a.per_frame_prob[tab[s * kSlotWords]];
				uint32_t j = i;
				while (j > 0) {
					const uint32_t sj = tab[(j - 1) * kSlotWords + 5];
					if (!cls_before(x, px, cls_load(tab, sj), a.per_frame_prob[tab[sj * kSlotWords]]))
						break;
					tab[j * kSlotWords + 5] = sj;
					--j;
				}
				tab[j * kSlotWords + 5] = s;
			}
			const ClsCounts f = cls_load(tab, tab[5]);
			ClsCounts r0 = f, r1 = f;
			for (int pass = 0; pass < 2; ++pass) {
				uint32_t n = 0;
				for (uint32_t i = 0; i < nv; ++i) {
					const uint32_t s = tab[i * kSlotWords + 5];
					const ClsCounts r = cls_load(tab, s);
					// isRoughlyEqualOrLarger(signifResults[0], candidate) (:347-356)
					if (!(cls_stderr_larger(f.count, r.count, a.extra_count) &&
					      cls_stderr_larger(f.totalNonSat, r.totalNonSat, a.extra_count) &&
					      cls_stderr_larger(f.nsFrame, r.nsFrame, a.extra_count) &&
					      cls_stderr_larger(f.solid, r.solid, a.extra_count) &&
					      cls_stderr_larger(f.nonSat, r.nonSat, a.extra_count) &&
					      cls_stderr_larger(f.total, r.total, a.extra_count)))
						continue;
					if (pass == 0) {
						if (n == 0)
							r0 = r;
						if (n == 1)
							r1 = r;
					} else if (n < a.max_results && lane == 0) {
						cls_write_hit<T>(a, row, n, tab[s * kSlotWords], r);
					}
					++n;
				}
				n_res = n;
				// checkCountAgreement (:358-364) of the first two
				if (pass == 0 && a.best_hit_agree && n >= 2 &&
				    !(r0.nsFrame >= r1.nsFrame && r0.count >= r1.count && r0.solid >= r1.solid && r0.nonSat >= r1.nonSat &&
				      r0.totalNonSat >= r1.totalNonSat && r0.total >= r1.total)) {
					n_res = 0;
					break;
				}
			}
		} else if (nv == 1) {
			const uint32_t s = tab[5];
			if (lane == 0)
				cls_write_hit<T>(a, row, 0, tab[s * kSlotWords], cls_load(tab, s));
			n_res = 1;
		}
	}
	if (lane == 0) {
		a.n_hits[row] = n_res;
		a.sat_count[row] = st.sat_count;
		a.eval_count[row] = st.eval;
	}
}

// the windows [b, e) of sequence s of the batch
__device__ __forceinline__ void cls_bounds(const MibfClassifyArgs& a, uint64_t s, uint64_t& b, uint64_t& e)
{
	if (a.layout.read_len) {
		b = s * a.layout.read_len;
		e = b + a.layout.read_len;
	} else {
		b = a.layout.starts[s];
		e = a.layout.starts[s + 1];
	}
}

} // namespace btlbf
