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
// The table, the per-frame body and the summary are in mibf_classify_core.hpp, shared with the walk over read pairs
// (mibf_classify_pair_kernels.hip).
#include "mibf_classify_core.hpp"

namespace btlbf {

// one sequence: windows [b, e) of the batch, result row `row`.  Every lane runs the same walk on the same values; the
// table is written with the same words by all of them.
template <class T>
__device__ __forceinline__ void cls_walk(const MibfClassifyArgs& a, uint32_t* tab, uint32_t cap, uint64_t b, uint64_t e,
                                         uint64_t row)
{
	ClsState st;
	for (uint64_t c = 0; cls_chunk_window(b, c) < e && !st.found; ++c) {
		uint32_t hm, v[kMibfMaxHash];
		uint64_t todo, mbits;
		cls_load_chunk<T>(a, cls_chunk_window(b, c), e, v, hm, todo, mbits);
		while (todo && !st.found) {
			const int src = __ffsll((unsigned long long)todo) - 1;
			todo &= todo - 1;
			if (!a.spaced)
				++st.eval; // ntHashIterator: ++m_evalCount per frame (:415)
			if (!((mbits >> src) & 1))
				continue;
			const uint32_t hits = __shfl(hm, src, 64);
			uint32_t fv[kMibfMaxHash];
#pragma unroll
			for (uint32_t i = 0; i < kMibfMaxHash; ++i)
				fv[i] = __shfl(v[i], src, 64);
			cls_frame<T>(a, tab, cap, st, hits, fv);
		}
	}
	cls_summarize<T>(a, tab, st, row);
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
