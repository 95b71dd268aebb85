// csrc/mibf_classify_pair_kernels.hip -- classification of read pairs: MIBFQuerySupport<T>::query(itr1, itr2, minCount)
// (MIBFQuerySupport.hpp:111-130) of every pair of a batch.  Sequences 2i and 2i + 1 of the batch are the mates of pair i.
//
// Phase 1 is the same MIBF_QUERY launch as for single reads, over the sequence layout (no window crosses a mate
// boundary).  Phase 2, here, is one walk over both mates' frames into ONE table with ONE early stop: at an even
// frameCount the next frame of mate 1 if it has one, else of mate 2; at an odd frameCount the other way round.
//   mibf_classify_pair_kernel<T, GLOBAL> : one wavefront per pair, every lane with the same state (the walk is serial,
//                                          mibf_classify_core.hpp).  Each mate is a frame source of its own: 64 loaded
//                                          windows and the ballot of those still to take.  Which source gives the next
//                                          frame is decided from wave-uniform values (frameCount and the two ballots),
//                                          so the wave never diverges on it.  The table has mibf_classify_cap() slots
//                                          for the pair's n1 + n2 bytes (frames1 + frames2 <= n1 + n2 - k + 1): in LDS
//                                          (GLOBAL = 0) up to kMibfClsLdsSlots, else in global scratch (GLOBAL = 1).
#include "mibf_classify_core.hpp"

namespace btlbf {

// the frames of one mate: windows [b, e), chunk c is the next to load; v / hm hold the loaded chunk's windows (one per
// lane), todo its frames not yet taken, mbits those of the chunk that hit
struct ClsSource {
	uint64_t b, e, c;
	uint32_t v[kMibfMaxHash], hm;
	uint64_t todo, mbits;
};

// load chunks until one holds a frame or the range is used up: afterwards todo == 0 means the mate is exhausted
template <class T>
__device__ __forceinline__ void cls_refill(const MibfClassifyArgs& a, ClsSource& s)
{
	while (s.todo == 0 && cls_chunk_window(s.b, s.c) < s.e) {
		cls_load_chunk<T>(a, cls_chunk_window(s.b, s.c), s.e, s.v, s.hm, s.todo, s.mbits);
		++s.c;
	}
}

// one pair: mate 1 is windows [b1, e1), mate 2 [b2, e2) of the batch; result row `row`
template <class T>
__device__ __forceinline__ void cls_walk_pair(const MibfClassifyArgs& a, uint32_t* tab, uint32_t cap, uint64_t b1,
                                              uint64_t e1, uint64_t b2, uint64_t e2, uint64_t row)
{
	ClsState st;
	ClsSource m1, m2;
	m1.b = b1, m1.e = e1, m1.c = 0, m1.todo = 0, m1.mbits = 0, m1.hm = 0;
	m2.b = b2, m2.e = e2, m2.c = 0, m2.todo = 0, m2.mbits = 0, m2.hm = 0;
#pragma unroll
	for (uint32_t i = 0; i < kMibfMaxHash; ++i)
		m1.v[i] = m2.v[i] = 0;
	cls_refill<T>(a, m1);
	cls_refill<T>(a, m2);
	uint32_t frame_count = 0;
	while ((m1.todo | m2.todo) && !st.found) {
		// :113-114 -- wave-uniform: todo comes from a ballot
		const bool second = (frame_count & 1) ? m2.todo != 0 : m1.todo == 0;
		++frame_count;
		const uint64_t todo = second ? m2.todo : m1.todo;
		const int src = __ffsll((unsigned long long)todo) - 1;
		const bool hit = ((second ? m2.mbits : m1.mbits) >> src) & 1;
		if (!a.spaced)
			++st.eval; // ntHashIterator: ++m_evalCount per frame (:415)
		if (hit) {
			const uint32_t hits = __shfl(second ? m2.hm : m1.hm, src, 64);
			uint32_t fv[kMibfMaxHash];
#pragma unroll
			for (uint32_t i = 0; i < kMibfMaxHash; ++i)
				fv[i] = __shfl(second ? m2.v[i] : m1.v[i], src, 64);
			cls_frame<T>(a, tab, cap, st, hits, fv);
		}
		if (second) {
			m2.todo &= m2.todo - 1;
			if (!st.found)
				cls_refill<T>(a, m2);
		} else {
			m1.todo &= m1.todo - 1;
			if (!st.found)
				cls_refill<T>(a, m1);
		}
	}
	cls_summarize<T>(a, tab, st, row);
}

// GLOBAL = 0: pair blockIdx * kClsWaves + wave of the batch, skipped when its table does not fit LDS;
// GLOBAL = 1 (one wave per workgroup): pair big_list[blockIdx], table at big_off[blockIdx] slots of big_tab
template <class T, int GLOBAL>
__global__ __launch_bounds__(GLOBAL ? 64 : 64 * kClsWaves) void mibf_classify_pair_kernel(const MibfClassifyArgs a)
{
	__shared__ uint32_t lds[GLOBAL ? 1 : kClsWaves][GLOBAL ? 1 : kMibfClsLdsSlots * kSlotWords];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint64_t p = GLOBAL ? 0 : (uint64_t)blockIdx.x * kClsWaves + wave;
	bool mine = GLOBAL ? true : p < a.layout.n_seqs / 2;
	if (GLOBAL)
		p = a.big_list[blockIdx.x];
	uint64_t b1 = 0, e1 = 0, b2 = 0, e2 = 0;
	uint32_t cap = 0;
	if (mine) {
		cls_bounds(a, 2 * p, b1, e1);
		cls_bounds(a, 2 * p + 1, b2, e2);
		cap = mibf_classify_cap(e2 - b1, a.k, a.h, a.n_ids); // the planner's expression: the mates are adjacent
		mine = GLOBAL ? true : cap <= kMibfClsLdsSlots;
	}
	uint32_t* tab = GLOBAL ? a.big_tab + a.big_off[blockIdx.x] * kSlotWords : lds[wave];
	if (mine)
		for (uint32_t i = lane; i < cap; i += 64)
			tab[i * kSlotWords] = kClsEmpty;
	__syncthreads(); // the cleared keys are visible to every lane of the wave (no wave has left yet)
	if (!mine)
		return;
	cls_walk_pair<T>(a, tab, cap, b1, e1, b2, e2, a.row0 + p);
	if (a.stat && lane == 0)
		atomicAdd(a.stat + (GLOBAL ? 1 : 0), 1ull);
}

// a.layout is the batch's sequence layout (n_seqs even), a.row0 the result row of its first pair, the big lists count
// pairs of the batch
hipError_t launch_mibf_classify_pairs(int id_bytes, const MibfClassifyArgs& a, hipStream_t s)
{
	const uint64_t n_pairs = a.layout.n_seqs / 2;
	if (n_pairs == 0)
		return hipSuccess;
	const uint64_t blocks = (n_pairs + kClsWaves - 1) / kClsWaves;
	if (a.h == 0 || a.h > kMibfMaxHash || (a.layout.n_seqs & 1) || blocks > 0x7fffffffull || a.n_big > 0x7fffffffull)
		return hipErrorInvalidValue;
	return mibf_by_id(id_bytes, [&](auto t) {
		using T = decltype(t);
		if (a.n_big < n_pairs) {
			hipLaunchKernelGGL((mibf_classify_pair_kernel<T, 0>), dim3((unsigned)blocks), dim3(64 * kClsWaves), 0, s, a);
			hipError_t e = hipGetLastError();
			if (e != hipSuccess)
				return e;
		}
		if (a.n_big)
			hipLaunchKernelGGL((mibf_classify_pair_kernel<T, 1>), dim3((unsigned)a.n_big), dim3(64), 0, s, a);
		return hipGetLastError();
	});
}

} // namespace btlbf
