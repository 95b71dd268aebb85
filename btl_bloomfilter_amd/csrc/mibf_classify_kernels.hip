// csrc/mibf_classify_kernels.hip -- read classification over the multi-index Bloom filter: MIBFQuerySupport<T>::query
// (MIBFQuerySupport.hpp:95-109) of every sequence of a batch.
//
// Phase 1 is mibf_seq_kernel<MIBF_QUERY> (mibf_kernels.hip): per window the raw T values, the match bit, the clean bit
// and the hit mask (m_hits of atRank).  Phase 2, here, walks each sequence's frames in order:
//   mibf_classify_kernel<T, GLOBAL> : one wavefront per sequence.  updatesCounts (:430-518) per hit frame with the early
//                                     stop of :102-105, then summarizeCandiates (:555-595).  The walk is serial (best /
//                                     second-best tracking, the stop), so every lane of the wave carries the same state
//                                     and the parallelism is across sequences; the wave loads 64 windows at a time and
//                                     hands the frames out by lane reads.  m_counts is an open-addressed table keyed by
//                                     ID, of mibf_classify_cap() slots (never n_ids entries): in LDS (GLOBAL = 0) when
//                                     that is at most kMibfClsLdsSlots, else in global scratch (GLOBAL = 1).
//   mibf_classify_maxid_kernel<T>   : the largest index the reference would use for m_counts over the whole data array
#include "internal.hpp"

namespace btlbf {

static constexpr uint32_t kClsEmpty = 0xffffffffu;
static constexpr uint32_t kClsWaves = 4; // sequences (wavefronts) per workgroup of the LDS kernel
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

// the slot of `id`, claimed and zeroed (m_counts[id] = {0,...}, :447-453) when the sequence meets the id for the first time.
// cap is a power of two above the number of distinct ids a sequence can meet, so an empty slot always exists.
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

// frame window: the frames of a sequence over [b, e) are its clean windows in position order; the walk takes them in
// chunks of 64 window starts, chunk c beginning here (the paired-read overload would alternate two such ranges)
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

// one sequence: windows [b, e) of the batch, result row `row`.  Every lane runs the same walk on the same values; the
// table is written with the same words by all of them.
template <class T>
__device__ __forceinline__ void cls_walk(const MibfClassifyArgs& a, uint32_t* tab, uint32_t cap, uint64_t b, uint64_t e,
                                         uint64_t row)
{
	constexpr uint32_t mask = ClsMask<T>::mask, anti = ClsMask<T>::anti;
	const uint32_t lane = threadIdx.x & 63u, h = a.h;
	const T* values = static_cast<const T*>(a.values);
	uint32_t n_cand = 0, sat_count = 0, eval = 0, extra = 0;
	uint32_t b_count = 0, b_nonsat = 0, b_total = 0, b_totalns = 0, b_nsf = 0, b_solid = 0, second = 0;
	bool found = false;

	for (uint64_t c = 0; cls_chunk_window(b, c) < e && !found; ++c) {
		const uint64_t gp = cls_chunk_window(b, c) + lane;
		bool ok = false, match = false;
		uint32_t hm = 0;
		uint32_t v[kMibfMaxHash];
#pragma unroll
		for (uint32_t i = 0; i < kMibfMaxHash; ++i)
			v[i] = 0;
		if (gp < e) {
			ok = (a.valid_bits[gp >> 6] >> (gp & 63)) & 1;
			match = (a.match_bits[gp >> 6] >> (gp & 63)) & 1;
			if (match) {
				hm = a.spaced ? a.hit_masks[gp] : (1u << h) - 1;
#pragma unroll
				for (uint32_t i = 0; i < kMibfMaxHash; ++i)
					if (i < h)
						v[i] = values[gp * h + i];
			}
		}
		uint64_t todo = __ballot(ok);
		const uint64_t mbits = __ballot(match);
		while (todo && !found) {
			const int src = __ffsll((unsigned long long)todo) - 1;
			todo &= todo - 1;
			if (!a.spaced)
				++eval; // ntHashIterator: ++m_evalCount per frame (:415)
			if (!((mbits >> src) & 1))
				continue;
			// ---- updatesCounts (:430-518) ----
			const uint32_t hits = __shfl(hm, src, 64);
			const uint32_t misses = h - __popc(hits);
			uint32_t fv[kMibfMaxHash], fslot[kMibfMaxHash];
#pragma unroll
			for (uint32_t i = 0; i < kMibfMaxHash; ++i) {
				fv[i] = __shfl(v[i], src, 64);
				fslot[i] = 0;
			}
			uint32_t seen = 0, fsat = 0; // seen: bit i = position i pushed its raw value onto m_seenSet
#pragma unroll
			for (uint32_t i = 0; i < kMibfMaxHash; ++i) {
				if (i >= h || !((hits >> i) & 1))
					continue;
				const uint32_t raw = fv[i];
				++eval;
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
				++sat_count;
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
				if (cr.count >= a.min_count_per_id[id] || (n_cand && cr.count >= b_count)) {
					if (tab[s * kSlotWords + 4] == 0) {
						tab[n_cand * kSlotWords + 5] = s;
						tab[s * kSlotWords + 4] = ++n_cand;
					}
					// updateMaxCounts (:520-542)
					if (cr.nsFrame > b_nsf)
						b_nsf = cr.nsFrame;
					else if (cr.nsFrame > second)
						second = cr.nsFrame;
					b_count = cr.count > b_count ? cr.count : b_count;
					b_nonsat = cr.nonSat > b_nonsat ? cr.nonSat : b_nonsat;
					b_solid = cr.solid > b_solid ? cr.solid : b_solid;
					b_total = cr.total > b_total ? cr.total : b_total;
					b_totalns = cr.totalNonSat > b_totalns ? cr.totalNonSat : b_totalns;
				}
			}
			if (cls_stderr(b_totalns, second))
				extra = 0;
			if (b_nsf > second) {
				if (a.extra_frame_limit < extra++)
					found = true;
			}
		}
	}

	// ---- summarizeCandiates (:555-595) ----
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
		a.sat_count[row] = sat_count;
		a.eval_count[row] = eval;
	}
}

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

// GLOBAL = 0: sequence blockIdx * kClsWaves + wave of the batch, skipped when its table does not fit LDS;
// GLOBAL = 1 (one wave per workgroup): sequence big_list[blockIdx], table at big_off[blockIdx] slots of big_tab
template <class T, int GLOBAL>
__global__ __launch_bounds__(GLOBAL ? 64 : 64 * kClsWaves) void mibf_classify_kernel(const MibfClassifyArgs a)
{
	__shared__ uint32_t lds[GLOBAL ? 1 : kClsWaves][GLOBAL ? 1 : kMibfClsLdsSlots * kSlotWords];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint64_t s = GLOBAL ? 0 : (uint64_t)blockIdx.x * kClsWaves + wave;
	bool mine = GLOBAL ? true : s < a.layout.n_seqs;
	if (GLOBAL)
		s = a.big_list[blockIdx.x];
	uint64_t b = 0, e = 0;
	uint32_t cap = 0;
	if (mine) {
		cls_bounds(a, s, b, e);
		cap = mibf_classify_cap(e - b, a.k, a.h, a.n_ids);
		mine = GLOBAL ? true : cap <= kMibfClsLdsSlots;
	}
	uint32_t* tab = GLOBAL ? a.big_tab + a.big_off[blockIdx.x] * kSlotWords : lds[wave];
	if (mine)
		for (uint32_t i = lane; i < cap; i += 64)
			tab[i * kSlotWords] = kClsEmpty;
	__syncthreads(); // the cleared keys are visible to every lane of the wave (no wave has left yet)
	if (!mine)
		return;
	cls_walk<T>(a, tab, cap, b, e, a.row0 + s);
	if (a.stat && lane == 0)
		atomicAdd(a.stat + (GLOBAL ? 1 : 0), 1ull);
}

// the index the reference uses for m_counts, minCount and perFrameProb (:442-456): the entry without its saturation
// bit when it is above the mask, else the entry itself (an entry EQUAL to the mask indexes as the mask)
template <class T>
__global__ __launch_bounds__(256) void mibf_classify_maxid_kernel(const T* data, uint64_t n, unsigned long long* out)
{
	uint32_t m = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t v = data[i];
		const uint32_t id = v > ClsMask<T>::mask ? v & ClsMask<T>::anti : v;
		m = id > m ? id : m;
	}
	for (int o = 32; o; o >>= 1) {
		const uint32_t x = __shfl_xor(m, o, 64);
		m = x > m ? x : m;
	}
	if ((threadIdx.x & 63) == 0 && m)
		atomicMax(out, (unsigned long long)m);
}

// ---- launchers ---------------------------------------------------------------------------------------------------

hipError_t launch_mibf_classify(int id_bytes, const MibfClassifyArgs& a, hipStream_t s)
{
	if (a.layout.n_seqs == 0)
		return hipSuccess;
	const uint64_t blocks = (a.layout.n_seqs + kClsWaves - 1) / kClsWaves;
	if (a.h == 0 || a.h > kMibfMaxHash || blocks > 0x7fffffffull || a.n_big > 0x7fffffffull)
		return hipErrorInvalidValue;
	return mibf_by_id(id_bytes, [&](auto t) {
		using T = decltype(t);
		if (a.n_big < a.layout.n_seqs) {
			hipLaunchKernelGGL((mibf_classify_kernel<T, 0>), dim3((unsigned)blocks), dim3(64 * kClsWaves), 0, s, a);
			hipError_t e = hipGetLastError();
			if (e != hipSuccess)
				return e;
		}
		if (a.n_big)
			hipLaunchKernelGGL((mibf_classify_kernel<T, 1>), dim3((unsigned)a.n_big), dim3(64), 0, s, a);
		return hipGetLastError();
	});
}

hipError_t launch_mibf_classify_maxid(int id_bytes, const void* data, uint64_t n, unsigned long long* out, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const uint64_t g = std::min<uint64_t>((n + 255) / 256, 4096);
	return mibf_by_id(id_bytes, [&](auto t) {
		using T = decltype(t);
		hipLaunchKernelGGL(mibf_classify_maxid_kernel<T>, dim3((unsigned)g), dim3(256), 0, s, static_cast<const T*>(data), n,
		                   out);
		return hipGetLastError();
	});
}

} // namespace btlbf
