// csrc/mibf_plan.hpp -- how the sequences of one miBF call are cut into batches under the scratch budget.  Plain integers
// and host arithmetic only (no HIP header): tests/cpp/test_mibf_plan.cpp includes it alone.  One rule serves insert, serial
// saturation and classify: cut [0, n_seqs) greedily into contiguous runs whose cost fits the budget, at least one sequence
// each; a sequence that does not fit alone fails the plan, before any batch has run.  Classifying read pairs plans the
// same way with the pair as its unit (mibf_plan_classify_pairs; tests/cpp/test_mibf_plan_pairs.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace btlbf {

// btlbf_mibf_set_scratch(0) means the default: a budget of 0 never reaches a planner
inline uint64_t mibf_budget(uint64_t set) { return set ? set : 2ull << 30; }

// read classification: a sequence's counts live in an open-addressed table of mibf_classify_cap() slots
static constexpr uint32_t kMibfClsSlotWords = 6;  // uint32_t per table slot
static constexpr uint32_t kMibfClsLdsSlots = 256; // tables up to this size are kept in LDS (6 KiB per wavefront)
// slots for a sequence of `bytes` bytes: a power of two above min(n_ids, windows * h), the distinct ids it can meet
// (constexpr: the kernels call it too)
constexpr uint32_t mibf_classify_cap(uint64_t bytes, uint32_t k, uint32_t h, uint64_t n_ids)
{
	const uint64_t frames = bytes >= k ? bytes - k + 1 : 0;
	uint64_t bound = frames * h;
	bound = bound < n_ids ? bound : n_ids;
	uint32_t cap = 16;
	while (cap <= bound && cap < 0x80000000u)
		cap <<= 1;
	return cap;
}

// the sequences of a call: a fixed read_len, or n_seqs + 1 host offsets
struct MibfSeqs {
	uint64_t n_seqs = 0;
	uint32_t read_len = 0;
	std::vector<uint64_t> starts;
	uint64_t start(uint64_t s) const { return read_len ? s * read_len : starts[s]; }
};
// what a sequence takes of the budget; slots != 0: it needs a global table of that many slots (classify)
struct MibfCost {
	uint64_t cost, slots;
};
struct MibfBatch {
	uint64_t s0, s1, big, slots; // sequences [s0, s1); how many of them need a global table, and the sum of their slots
};
struct MibfPlan {
	std::vector<MibfBatch> batches;
	// the sequences with a global table, batch after batch: index in the batch, first slot of the table in the batch's
	std::vector<uint32_t> big_seq;
	std::vector<uint64_t> big_off;
	uint64_t max_bytes = 0, max_big = 0, max_slots = 0; // the largest batch in each respect: what scratch is sized from
	uint64_t too_big = ~0ull;                           // the first sequence that does not fit the budget alone
	bool ok() const { return too_big == ~0ull; }
};

// cost(bytes) -> MibfCost of a sequence of that length; at most max_seqs sequences per batch
template <class Cost>
MibfPlan mibf_plan(const MibfSeqs& q, uint64_t budget, uint64_t max_seqs, Cost cost)
{
	MibfPlan p;
	// a fixed read_len: every sequence costs the same, so the size of a batch is computed once; only sequences with a
	// global table are walked one by one, for their places in the batch's lists
	const MibfCost fixed = q.read_len ? cost(q.read_len) : MibfCost{0, 0};
	const uint64_t per_batch = fixed.cost ? std::min(max_seqs, budget / fixed.cost) : max_seqs;
	for (uint64_t s0 = 0; s0 < q.n_seqs;) {
		MibfBatch b{s0, s0, 0, 0};
		if (q.read_len && !fixed.slots) {
			b.s1 = s0 + std::min(per_batch, q.n_seqs - s0);
		} else {
			for (uint64_t used = 0; b.s1 < q.n_seqs && b.s1 - s0 < max_seqs; ++b.s1) {
				const MibfCost c = q.read_len ? fixed : cost(q.starts[b.s1 + 1] - q.starts[b.s1]);
				if (c.cost > budget - used)
					break;
				used += c.cost;
				if (c.slots) {
					p.big_seq.push_back((uint32_t)(b.s1 - s0));
					p.big_off.push_back(b.slots);
					++b.big;
					b.slots += c.slots;
				}
			}
		}
		if (b.s1 == s0) {
			p.too_big = s0;
			return p;
		}
		p.max_bytes = std::max(p.max_bytes, q.start(b.s1) - q.start(s0));
		p.max_big = std::max(p.max_big, b.big);
		p.max_slots = std::max(p.max_slots, b.slots);
		p.batches.push_back(b);
		s0 = b.s1;
	}
	return p;
}

inline MibfCost mibf_cost_bytes(uint64_t n) { return MibfCost{n, 0}; }
// insert IDs: 4 x 8 bytes per hash value (keys, values, and the sort's output) + the sort's scratch
inline MibfPlan mibf_plan_insert(const MibfSeqs& q, uint64_t budget, uint32_t h)
{
	return mibf_plan(q, std::max<uint64_t>(1, budget / (40ull * h)), ~0ull, mibf_cost_bytes);
}
// serial saturation: the hash rows of a batch, 8 bytes per hash value + the window bitmap
inline MibfPlan mibf_plan_serial(const MibfSeqs& q, uint64_t budget, uint32_t h)
{
	return mibf_plan(q, std::max<uint64_t>(1, budget / (8ull * h + 1)), ~0ull, mibf_cost_bytes);
}
// parallel saturation decides a whole batch against one snapshot, so it is not cut: its two lists take half of the budget
// each -- a mutation 40 bytes ((rank, window) and as much for their sort, as an insert's hash value), a saturated rank 8.
inline uint64_t mibf_parallel_cap_mut(uint64_t budget) { return budget / 2 / 40; }
inline uint64_t mibf_parallel_cap_sat(uint64_t budget) { return budget / 2 / 8; }
// the windows a batch of whole records of `bytes` bytes can hold: one record of all of them
inline uint64_t mibf_batch_windows(uint64_t bytes, uint32_t k) { return bytes >= k ? bytes - k + 1 : 0; }
// the worst case of a batch of `windows` windows fits: every window a mutation (one entry), or every window a saturation
// (h ranks)
inline bool mibf_parallel_fits(uint64_t windows, uint32_t h, uint64_t budget)
{
	return windows <= mibf_parallel_cap_mut(budget) && windows <= mibf_parallel_cap_sat(budget) / h;
}
// ... and the smallest budget under which it does (~0 where that is beyond 64 bits)
inline uint64_t mibf_parallel_budget(uint64_t windows, uint32_t h)
{
	const uint64_t per = std::max<uint64_t>(80, 16ull * h);
	return windows > ~0ull / per ? ~0ull : windows * per;
}
// the longest record one insert batch (serial: one serial saturation batch) holds, and the smallest budget that holds
// `bytes` >= 2 (a batch always has room for one byte): the planners above, read backwards
inline uint64_t mibf_record_room(uint64_t budget, uint32_t h, bool serial)
{
	return std::max<uint64_t>(1, budget / (serial ? 8ull * h + 1 : 40ull * h));
}
inline uint64_t mibf_record_budget(uint64_t bytes, uint32_t h, bool serial)
{
	const uint64_t per = serial ? 8ull * h + 1 : 40ull * h;
	return bytes > ~0ull / per ? ~0ull : bytes * per;
}

// classify: per byte h values, the hit mask and two bitmap bits; per sequence whose table does not fit LDS, the table
inline MibfPlan mibf_plan_classify(const MibfSeqs& q, uint64_t budget, uint32_t k, uint32_t h, uint32_t id_bytes,
                                   uint64_t n_ids)
{
	return mibf_plan(q, budget, 0x7fffffffull, [=](uint64_t n) {
		const uint32_t cap = mibf_classify_cap(n, k, h, n_ids);
		const uint64_t slots = cap > kMibfClsLdsSlots ? cap : 0;
		return MibfCost{n * ((uint64_t)h * id_bytes + 2) + 64 + slots * kMibfClsSlotWords * 4 + (slots ? 12 : 0), slots};
	});
}

// classify pairs: sequences 2i and 2i + 1 of q (n_seqs even) are the mates of pair i.  The unit is the pair, so no batch
// separates two mates: the plan's s0, s1, big_seq and too_big count PAIRS, and a batch is sequences [2 * s0, 2 * s1).
// The mates are adjacent in the buffer, so a pair is one range of n = n1 + n2 bytes; its table has
// mibf_classify_cap(n, ...) slots (frames1 + frames2 <= n - k + 1).  Per pair: the bytes of phase 1 as for single reads,
// 128 bytes for the two sequences' share of the layout and the result rows, and its table when that does not fit LDS.
inline MibfPlan mibf_plan_classify_pairs(const MibfSeqs& q, uint64_t budget, uint32_t k, uint32_t h, uint32_t id_bytes,
                                         uint64_t n_ids)
{
	MibfSeqs pairs;
	pairs.n_seqs = q.n_seqs / 2;
	if (q.read_len && q.read_len <= 0x7fffffffu) {
		pairs.read_len = 2 * q.read_len;
	} else {
		pairs.starts.resize(pairs.n_seqs + 1);
		for (uint64_t i = 0; i <= pairs.n_seqs; ++i)
			pairs.starts[i] = q.read_len ? 2 * i * q.read_len : q.starts[2 * i];
	}
	return mibf_plan(pairs, budget, 0x3fffffffull, [=](uint64_t n) {
		const uint32_t cap = mibf_classify_cap(n, k, h, n_ids);
		const uint64_t slots = cap > kMibfClsLdsSlots ? cap : 0;
		return MibfCost{n * ((uint64_t)h * id_bytes + 2) + 128 + slots * kMibfClsSlotWords * 4 + (slots ? 12 : 0), slots};
	});
}

} // namespace btlbf
