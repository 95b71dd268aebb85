// The pair planner (mibf_plan_classify_pairs, csrc/mibf_plan.hpp) against a brute-force planner written from its
// contract: the unit is the pair (sequences 2i, 2i + 1), batches cover every pair once and in order and never separate
// two mates, their cost stays within the budget and they are maximal, the first pair that does not fit alone fails the
// plan, and the global-table lists point at the right pairs.  Random ragged and fixed layouts, the edges, and the plan of
// the GPU test "a long mate takes the global table" (tests/test_gpu_mibf_classify_pairs.py, same lengths and budget).
// Built with -fsanitize=address,undefined by tests/test_mibf_plan_pairs_cpu.py; includes nothing but that header.
#include "../../btl_bloomfilter_amd/csrc/mibf_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace btlbf;

static unsigned long long g_case = 0;
#define CHECK(c)                                                                                        \
	do {                                                                                                \
		if (!(c)) {                                                                                     \
			fprintf(stderr, "%s:%d: CHECK(%s) failed in case %llu\n", __FILE__, __LINE__, #c, g_case); \
			exit(1);                                                                                    \
		}                                                                                               \
	} while (0)

struct Rule {
	uint32_t h, k, id_bytes;
	uint64_t n_ids;
};

// the rules as the C ABI documents them, restated without the header's functions
static_assert(kMibfClsLdsSlots == 256 && kMibfClsSlotWords == 6, "the restatement below uses these");
static uint64_t ref_slots(uint64_t n, const Rule& r)
{
	const uint64_t frames = n >= r.k ? n - r.k + 1 : 0;
	const uint64_t bound = std::min<uint64_t>(frames * r.h, r.n_ids);
	uint64_t cap = 16;
	while (cap <= bound)
		cap *= 2;
	return cap > 256 ? cap : 0;
}
static uint64_t ref_cost(uint64_t n, const Rule& r)
{
	const uint64_t slots = ref_slots(n, r);
	return n * (r.h * r.id_bytes + 2) + 128 + slots * 6 * 4 + (slots ? 12 : 0);
}

struct RefBatch {
	uint64_t p0, p1;
	std::vector<uint32_t> big;     // pairs of the batch with a global table
	std::vector<uint64_t> big_off; // and the first slot of each
	uint64_t slots, bytes;
};
// greedy, pair by pair; returns the first pair that does not fit alone, or ~0
static uint64_t brute(const std::vector<uint64_t>& lens, uint64_t budget, const Rule& r, std::vector<RefBatch>& out)
{
	const uint64_t n_pairs = lens.size() / 2;
	for (uint64_t p = 0; p < n_pairs;) {
		RefBatch b{p, p, {}, {}, 0, 0};
		uint64_t used = 0;
		while (b.p1 < n_pairs) {
			const uint64_t n = lens[2 * b.p1] + lens[2 * b.p1 + 1], c = ref_cost(n, r);
			if (used + c > budget)
				break;
			used += c;
			if (const uint64_t s = ref_slots(n, r)) {
				b.big.push_back((uint32_t)(b.p1 - p));
				b.big_off.push_back(b.slots);
				b.slots += s;
			}
			b.bytes += n;
			++b.p1;
		}
		if (b.p1 == p)
			return p;
		out.push_back(b);
		p = b.p1;
	}
	return ~0ull;
}

static MibfSeqs ragged(const std::vector<uint64_t>& lens)
{
	MibfSeqs q;
	q.n_seqs = lens.size();
	q.starts.assign(1, 0);
	for (uint64_t n : lens)
		q.starts.push_back(q.starts.back() + n);
	return q;
}

static void check(const std::vector<uint64_t>& lens, const MibfPlan& p, uint64_t budget, const Rule& r)
{
	std::vector<RefBatch> ref;
	const uint64_t bad = brute(lens, budget, r, ref);
	CHECK(p.ok() == (bad == ~0ull));
	CHECK(p.too_big == bad);
	if (!p.ok())
		return;
	CHECK(p.batches.size() == ref.size());
	uint64_t at = 0, big_at = 0, max_bytes = 0, max_big = 0, max_slots = 0;
	for (size_t i = 0; i < ref.size(); ++i) {
		const MibfBatch& b = p.batches[i];
		// in pairs: sequences [2 * s0, 2 * s1), so no batch begins or ends between two mates
		CHECK(b.s0 == at && b.s0 == ref[i].p0 && b.s1 == ref[i].p1 && b.s1 > b.s0 && 2 * b.s1 <= lens.size());
		CHECK(b.big == ref[i].big.size() && b.slots == ref[i].slots);
		uint64_t cost = 0;
		for (uint64_t q = b.s0; q < b.s1; ++q)
			cost += ref_cost(lens[2 * q] + lens[2 * q + 1], r);
		CHECK(cost <= budget);
		for (size_t j = 0; j < ref[i].big.size(); ++j, ++big_at) {
			CHECK(big_at < p.big_seq.size() && p.big_seq.size() == p.big_off.size());
			CHECK(p.big_seq[big_at] == ref[i].big[j] && p.big_off[big_at] == ref[i].big_off[j]);
			const uint64_t q = b.s0 + p.big_seq[big_at];
			CHECK(ref_slots(lens[2 * q] + lens[2 * q + 1], r) > 256); // the pair it points at needs a global table
		}
		max_bytes = std::max(max_bytes, ref[i].bytes);
		max_big = std::max<uint64_t>(max_big, ref[i].big.size());
		max_slots = std::max(max_slots, ref[i].slots);
		at = b.s1;
	}
	CHECK(2 * at == lens.size() && big_at == p.big_seq.size());
	CHECK(p.max_bytes == max_bytes && p.max_big == max_big && p.max_slots == max_slots);
}

static void same(const MibfPlan& a, const MibfPlan& b)
{
	CHECK(a.too_big == b.too_big && a.batches.size() == b.batches.size());
	for (size_t i = 0; i < a.batches.size(); ++i)
		CHECK(a.batches[i].s0 == b.batches[i].s0 && a.batches[i].s1 == b.batches[i].s1 && a.batches[i].big == b.batches[i].big &&
		      a.batches[i].slots == b.batches[i].slots);
	CHECK(a.big_seq == b.big_seq && a.big_off == b.big_off);
	CHECK(a.max_bytes == b.max_bytes && a.max_big == b.max_big && a.max_slots == b.max_slots);
}

static MibfPlan run(const MibfSeqs& q, uint64_t budget, const Rule& r)
{
	return mibf_plan_classify_pairs(q, budget, r.k, r.h, r.id_bytes, r.n_ids);
}

static void random_cases(unsigned n_cases, std::mt19937_64& rng)
{
	auto rnd = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
	const uint64_t n_ids_of[] = {1, 10, 100, 255, 256, 257, 300, 1000, 40000};
	for (unsigned c = 0; c < n_cases; ++c, ++g_case) {
		const Rule r{(uint32_t)rnd(1, 8), (uint32_t)rnd(20, 40), rnd(0, 1) ? 2u : 4u, n_ids_of[rnd(0, 8)]};
		const uint64_t n_pairs = rnd(0, 24);
		const bool fixed = rnd(0, 2) == 0;
		const uint64_t L = rnd(1, 400);
		std::vector<uint64_t> lens;
		for (uint64_t i = 0; i < 2 * n_pairs; ++i) { // empty mates, mates shorter than k, anything
			const uint64_t what = rnd(0, 5);
			lens.push_back(fixed ? L : what == 0 ? 0 : what == 1 ? rnd(1, r.k - 1) : rnd(0, 400));
		}
		uint64_t most = 0, total = 0;
		for (uint64_t i = 0; i < n_pairs; ++i) {
			const uint64_t x = ref_cost(lens[2 * i] + lens[2 * i + 1], r);
			most = std::max(most, x);
			total += x;
		}
		uint64_t budget = 1; // from too small for anything, around the largest pair, a few batches, to everything
		switch (rnd(0, 5)) {
		case 0: budget = rnd(1, 200); break;
		case 1: budget = most ? most - rnd(0, 1) : 1; break;
		case 2: budget = most + rnd(0, 2); break;
		case 3: budget = rnd(1, most + 2); break;
		case 4: budget = most + rnd(0, total / 3 + 1); break;
		default: budget = total + rnd(0, 10); break;
		}
		const MibfPlan p = run(ragged(lens), budget, r);
		check(lens, p, budget, r);
		if (fixed) { // a fixed read_len cuts where the same offsets cut
			MibfSeqs f;
			f.n_seqs = 2 * n_pairs;
			f.read_len = (uint32_t)L;
			const MibfPlan pf = run(f, budget, r);
			check(lens, pf, budget, r);
			same(p, pf);
		}
	}
}

static void edges()
{
	++g_case;
	const Rule r{4, 31, 2, 301};
	// no pair: an empty plan, for both layouts
	MibfSeqs none = ragged({}), none_fixed;
	none_fixed.read_len = 100;
	for (const MibfSeqs* q : {&none, &none_fixed}) {
		const MibfPlan p = run(*q, 1, r);
		CHECK(p.ok() && p.batches.empty() && p.max_bytes == 0 && p.max_big == 0 && p.max_slots == 0);
	}
	// one pair exactly at the budget, and one byte over: the two mates count together, however the bytes are split
	const uint64_t exact = ref_cost(300, r);
	for (uint64_t n1 : {0ull, 1ull, 150ull, 300ull}) {
		MibfPlan p = run(ragged({n1, 300 - n1}), exact, r);
		check({n1, 300 - n1}, p, exact, r);
		CHECK(p.ok() && p.batches.size() == 1 && p.batches[0].s0 == 0 && p.batches[0].s1 == 1 && p.max_bytes == 300);
		p = run(ragged({n1, 301 - n1}), exact, r);
		CHECK(!p.ok() && p.too_big == 0);
	}
	// each mate alone would fit, the pair does not: the plan fails at that pair (counted in pairs), not at a sequence
	MibfPlan p = run(ragged({100, 200, 0, 0, 200, 101, 10, 10}), exact, r);
	check({100, 200, 0, 0, 200, 101, 10, 10}, p, exact, r);
	CHECK(!p.ok() && p.too_big == 2);
	// a table is sized for both mates: two mates of 40 bases over 301 ids stay in LDS (50 frames * 4 < 256), two of 60 do not
	CHECK(mibf_classify_cap(80, 31, 4, 301) == 256 && mibf_classify_cap(120, 31, 4, 301) == 512);
	p = run(ragged({40, 40, 60, 60}), mibf_budget(0), r);
	check({40, 40, 60, 60}, p, mibf_budget(0), r);
	CHECK(p.ok() && p.batches.size() == 1 && p.batches[0].big == 1 && p.big_seq[0] == 1 && p.big_off[0] == 0 && p.max_slots == 512);
	// a read_len whose double does not fit 32 bits is planned from offsets
	MibfSeqs big;
	big.n_seqs = 2;
	big.read_len = 0x90000000u;
	p = run(big, ~0ull, r);
	CHECK(p.ok() && p.batches.size() == 1 && p.max_bytes == 2ull * 0x90000000u);
}

// tests/test_gpu_mibf_classify_pairs.py::test_a_long_mate_takes_the_global_table: the pairs (46, 46) and (80, 5000), 301
// table entries, C5 seeds (h = 4, k = 31), uint16 ids, budget 64000
static void gpu_case()
{
	++g_case;
	const Rule r{4, 31, 2, 301};
	const std::vector<uint64_t> lens = {46, 46, 80, 5000};
	CHECK(ref_cost(92, r) == 1048 && ref_slots(92, r) == 0 && ref_cost(5080, r) == 63228);
	const MibfPlan p = run(ragged(lens), 64000, r);
	check(lens, p, 64000, r);
	CHECK(p.ok() && p.batches.size() == 2);
	CHECK(p.batches[0].s0 == 0 && p.batches[0].s1 == 1 && p.batches[0].big == 0);
	CHECK(p.batches[1].s0 == 1 && p.batches[1].s1 == 2 && p.batches[1].big == 1 && p.batches[1].slots == 512);
	CHECK(p.big_seq.size() == 1 && p.big_seq[0] == 0 && p.big_off[0] == 0);
	CHECK(p.max_bytes == 5080 && p.max_big == 1 && p.max_slots == 512);
}

int main()
{
	std::mt19937_64 rng(20261019);
	random_cases(6000, rng);
	edges();
	gpu_case();
	printf("mibf pair plan test passed: %llu cases\n", g_case);
	return 0;
}
