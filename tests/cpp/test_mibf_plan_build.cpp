// tests/cpp/test_mibf_plan_build.cpp -- TEST-ONLY: the miBF builder's bounds (csrc/mibf_plan.hpp) against brute force.
// Parallel saturation decides a whole batch in one call whose two lists get half of the scratch budget each (a mutation
// 40 bytes, a saturated rank 8): a batch of W windows fits when W mutations and W * h saturated ranks both fit, and
// mibf_parallel_budget is the SMALLEST budget under which they do.  The record bounds are the insert / serial planners
// read backwards: a record fits exactly when the planner plans it, and mibf_record_budget is the smallest such budget.
#include "../../btl_bloomfilter_amd/csrc/mibf_plan.hpp"

#include <cstdio>

using namespace btlbf;

static int g_fail = 0;
#define EXPECT(cond)                                                                                                   \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			if (++g_fail < 20)                                                                                         \
				std::fprintf(stderr, "line %d: %s (w %llu h %u budget %llu)\n", __LINE__, #cond, (unsigned long long)w, h, \
				             (unsigned long long)budget);                                                              \
		}                                                                                                              \
	} while (0)

int main()
{
	// the parallel bound: every (windows, h, budget) of a small grid, against the two lists' capacities spelled out
	for (uint64_t w = 0; w <= 40; ++w)
		for (uint32_t h = 1; h <= 8; ++h) {
			uint64_t smallest = ~0ull;
			for (uint64_t budget = 0; budget <= 40 * 16 * 8 + 200; ++budget) {
				const uint64_t cap_mut = (budget / 2) / 40, cap_sat = (budget / 2) / 8;
				const bool fits = w <= cap_mut && w * h <= cap_sat;
				EXPECT(mibf_parallel_fits(w, h, budget) == fits);
				EXPECT(mibf_parallel_cap_mut(budget) == cap_mut && mibf_parallel_cap_sat(budget) == cap_sat);
				if (fits && smallest == ~0ull)
					smallest = budget;
			}
			const uint64_t budget = mibf_parallel_budget(w, h);
			EXPECT(budget == smallest);
			EXPECT(mibf_parallel_fits(w, h, budget) && (budget == 0 || !mibf_parallel_fits(w, h, budget - 1)));
		}
	// the windows of a batch of whole records: one record of all its bytes
	for (uint64_t w = 0; w <= 100; ++w)
		for (uint32_t h = 1; h <= 70; ++h) { // (w: bytes, h: k)
			const uint64_t budget = 0;
			uint64_t most = 0;
			for (uint64_t first = 0; first <= w; ++first) { // two records of first and w - first bytes
				const uint64_t a = first >= h ? first - h + 1 : 0, b = w - first >= h ? w - first - h + 1 : 0;
				most = a + b > most ? a + b : most;
			}
			EXPECT(mibf_batch_windows(w, h) == most);
		}
	// the record bounds: a record of w bytes alone, planned
	for (int serial = 0; serial < 2; ++serial)
		for (uint32_t h = 1; h <= 8; ++h)
			for (uint64_t w = 0; w <= 30; ++w) {
				uint64_t smallest = ~0ull;
				for (uint64_t budget = 1; budget <= 30 * 40 * 8 + 50; ++budget) {
					MibfSeqs q;
					q.n_seqs = 1;
					q.starts = {0, w};
					const bool planned = (serial ? mibf_plan_serial(q, budget, h) : mibf_plan_insert(q, budget, h)).ok();
					EXPECT((w <= mibf_record_room(budget, h, serial)) == planned);
					if (planned && smallest == ~0ull)
						smallest = budget;
				}
				const uint64_t budget = mibf_record_budget(w, h, serial);
				// the planners give every batch room for at least one byte, so a record of 0 or 1 bytes fits any budget (and a
				// budget of 0 is the default: it never reaches a planner)
				EXPECT(smallest == (w <= 1 ? 1 : budget));
			}
	// beyond 64 bits: no wrap
	{
		const uint64_t w = ~0ull / 16, budget = 0;
		const uint32_t h = 8;
		EXPECT(mibf_parallel_budget(w, h) == ~0ull && mibf_record_budget(w, h, false) == ~0ull);
	}
	if (g_fail) {
		std::printf("%d checks failed\n", g_fail);
		return 1;
	}
	std::printf("mibf build plan test passed\n");
	return 0;
}
