// The miBF batch planner (csrc/mibf_plan.hpp) against a brute-force restatement of its contract: random small cases
// per cost rule, the edges, and the plan of the GPU test "global table in a later batch"
// (tests/test_gpu_mibf_classify.py, same lengths and budget).  Built with -fsanitize=address,undefined by
// tests/test_mibf_plan_cpu.py; includes nothing of the library but that header.
#include "../../btl_bloomfilter_amd/csrc/mibf_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace btlbf;

static unsigned long long g_case = 0;
#define CHECK(c)                                                                                          \
	do {                                                                                                  \
		if (!(c)) {                                                                                       \
			fprintf(stderr, "%s:%d: CHECK(%s) failed in case %llu\n", __FILE__, __LINE__, #c, g_case);   \
			exit(1);                                                                                      \
		}                                                                                                 \
	} while (0)

enum Kind { INSERT, SERIAL, CLASSIFY, CAPPED };
struct Rule {
	Kind kind;
	uint32_t h, k, id_bytes;
	uint64_t n_ids, cap; // cap: CAPPED only (bytes cost, at most cap sequences per batch)
};

// the rules as the C ABI documents them, restated without the header's functions
static_assert(kMibfClsLdsSlots == 256 && kMibfClsSlotWords == 6, "the restatement below uses these");
static uint64_t ref_slots(uint64_t n, const Rule& r)
{
	if (r.kind != CLASSIFY)
		return 0;
	const uint64_t frames = n >= r.k ? n - r.k + 1 : 0;
	const uint64_t bound = std::min<uint64_t>(frames * r.h, r.n_ids);
	uint64_t cap = 16;
	while (cap <= bound)
		cap *= 2;
	return cap > 256 ? cap : 0;
}
static uint64_t ref_cost(uint64_t n, const Rule& r)
{
	if (r.kind != CLASSIFY)
		return n;
	const uint64_t slots = ref_slots(n, r);
	return n * (r.h * r.id_bytes + 2) + 64 + slots * 6 * 4 + (slots ? 12 : 0);
}
static uint64_t ref_divisor(const Rule& r) { return r.kind == INSERT ? 40ull * r.h : r.kind == SERIAL ? 8ull * r.h + 1 : 1; }
static uint64_t ref_budget(uint64_t budget, const Rule& r) { return std::max<uint64_t>(1, budget / ref_divisor(r)); }
static uint64_t ref_cap(const Rule& r) { return r.kind == CLASSIFY ? 0x7fffffffull : r.kind == CAPPED ? r.cap : ~0ull; }

static MibfPlan run(const MibfSeqs& q, uint64_t budget, const Rule& r)
{
	switch (r.kind) {
	case INSERT: return mibf_plan_insert(q, budget, r.h);
	case SERIAL: return mibf_plan_serial(q, budget, r.h);
	case CLASSIFY: return mibf_plan_classify(q, budget, r.k, r.h, r.id_bytes, r.n_ids);
	default: return mibf_plan(q, budget, r.cap, [](uint64_t n) { return MibfCost{n, 0}; });
	}
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
	const uint64_t n = lens.size(), eff = ref_budget(budget, r), cap = ref_cap(r);
	uint64_t bad = ~0ull;
	for (uint64_t i = 0; i < n && bad == ~0ull; ++i)
		if (ref_cost(lens[i], r) > eff)
			bad = i;
	CHECK(p.ok() == (bad == ~0ull));
	CHECK(p.too_big == bad);
	if (!p.ok())
		return;
	uint64_t at = 0, big_at = 0, max_bytes = 0, max_big = 0, max_slots = 0;
	for (const MibfBatch& b : p.batches) {
		CHECK(b.s0 == at && b.s1 > b.s0 && b.s1 <= n && b.s1 - b.s0 <= cap);
		uint64_t cost = 0, bytes = 0, big = 0, slots = 0;
		for (uint64_t i = b.s0; i < b.s1; ++i) {
			cost += ref_cost(lens[i], r);
			bytes += lens[i];
			if (const uint64_t s = ref_slots(lens[i], r)) {
				CHECK(big_at < p.big_seq.size() && p.big_seq.size() == p.big_off.size());
				CHECK(p.big_seq[big_at] == i - b.s0 && p.big_off[big_at] == slots);
				++big_at;
				++big;
				slots += s;
			}
		}
		CHECK(cost <= eff);
		CHECK(b.big == big && b.slots == slots);
		if (b.s1 < n) // maximal: the next sequence would not have fitted
			CHECK(cost + ref_cost(lens[b.s1], r) > eff || b.s1 - b.s0 == cap);
		max_bytes = std::max(max_bytes, bytes);
		max_big = std::max(max_big, big);
		max_slots = std::max(max_slots, slots);
		at = b.s1;
	}
	CHECK(at == n && big_at == p.big_seq.size());
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

static void random_cases(Kind kind, unsigned n_cases, std::mt19937_64& rng)
{
	auto rnd = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
	const uint64_t n_ids_of[] = {1, 10, 100, 255, 256, 257, 300, 1000, 40000};
	for (unsigned c = 0; c < n_cases; ++c, ++g_case) {
		Rule r{kind, (uint32_t)rnd(1, 8), (uint32_t)rnd(20, 40), rnd(0, 1) ? 2u : 4u, n_ids_of[rnd(0, 8)], rnd(1, 5)};
		const uint64_t n = rnd(0, 40);
		const bool fixed = rnd(0, 2) == 0;
		const uint64_t L = rnd(1, 400);
		std::vector<uint64_t> lens;
		for (uint64_t i = 0, run = 0, run_len = 0; i < n; ++i) {
			if (run == 0) { // runs of empty sequences, of sequences shorter than k, of anything
				run = rnd(1, 6);
				const uint64_t what = rnd(0, 5);
				run_len = what == 0 ? 0 : what == 1 ? rnd(1, r.k - 1) : ~0ull;
			}
			--run;
			lens.push_back(fixed ? L : run_len != ~0ull ? run_len : rnd(0, 400));
		}
		uint64_t most = 0, total = 0;
		for (uint64_t x : lens) {
			most = std::max(most, ref_cost(x, r));
			total += ref_cost(x, r);
		}
		uint64_t target = 1; // the effective budget aimed at: from 1 unit up, around the largest sequence, a few batches, all
		switch (rnd(0, 5)) {
		case 0: target = rnd(1, 3); break;
		case 1: target = most ? most - rnd(0, 1) : 1; break;
		case 2: target = most + rnd(0, 2); break;
		case 3: target = rnd(1, most + 2); break;
		case 4: target = most + rnd(0, total / 3 + 1); break;
		default: target = total + rnd(0, 10); break;
		}
		const uint64_t budget = std::max<uint64_t>(1, target * ref_divisor(r) + rnd(0, ref_divisor(r) - 1));
		const MibfSeqs q = ragged(lens);
		const MibfPlan p = run(q, budget, r);
		check(lens, p, budget, r);
		if (fixed) { // the computed batch size of a fixed read_len cuts where the walk over the same offsets cuts
			MibfSeqs f;
			f.n_seqs = n;
			f.read_len = (uint32_t)L;
			const MibfPlan pf = run(f, budget, r);
			check(lens, pf, budget, r);
			same(p, pf);
		}
	}
}

static void edges()
{
	const Rule rules[] = {{INSERT, 4, 31, 2, 100, 0}, {SERIAL, 3, 31, 4, 100, 0}, {CLASSIFY, 4, 31, 2, 301, 0},
	                      {CAPPED, 1, 31, 2, 1, 2}};
	for (const Rule& r : rules) {
		++g_case;
		// no sequence: an empty plan, for both layouts
		MibfSeqs none = ragged({}), none_fixed;
		none_fixed.read_len = 100;
		for (const MibfSeqs* q : {&none, &none_fixed}) {
			const MibfPlan p = run(*q, 1, r);
			CHECK(p.ok() && p.batches.empty() && p.max_bytes == 0 && p.max_big == 0 && p.max_slots == 0);
		}
		// one sequence exactly at the budget, and one byte over
		const uint64_t n = 300, exact = ref_cost(n, r) * ref_divisor(r);
		CHECK(ref_budget(exact, r) == ref_cost(n, r));
		MibfPlan p = run(ragged({n}), exact, r);
		check({n}, p, exact, r);
		CHECK(p.ok() && p.batches.size() == 1 && p.max_bytes == n);
		p = run(ragged({n + 1}), exact, r);
		check({n + 1}, p, exact, r);
		CHECK(!p.ok() && p.too_big == 0);
		p = run(ragged({n, 0, n + 1, n + 1}), exact, r);
		CHECK(!p.ok() && p.too_big == 2);
		// budget 0 is the API's word for the default: mibf_budget() is what the callers hand on, never 0
		CHECK(mibf_budget(0) == 2ull << 30 && mibf_budget(1) == 1 && mibf_budget(12345) == 12345);
		p = run(ragged({n, n, n}), mibf_budget(0), r);
		check({n, n, n}, p, mibf_budget(0), r);
		CHECK(p.ok() && p.batches.size() == (r.kind == CAPPED ? 2u : 1u));
	}
}

// tests/test_gpu_mibf_classify.py::test_global_table_in_a_later_batch: three 80-base reads, then one of 5000 bases, 301
// table entries, C5 seeds (h = 4, k = 31), uint16 ids, budget 63000
static void gpu_case()
{
	++g_case;
	const Rule r{CLASSIFY, 4, 31, 2, 301, 0};
	const std::vector<uint64_t> lens = {80, 80, 80, 5000};
	const uint64_t budget = 63000;
	const MibfPlan p = run(ragged(lens), budget, r);
	check(lens, p, budget, r);
	CHECK(p.ok() && p.batches.size() == 2);
	CHECK(p.batches[0].s1 == 3 && p.batches[0].big == 0);
	CHECK(p.batches[1].s0 == 3 && p.batches[1].s1 == 4 && p.batches[1].big == 1 && p.batches[1].slots == 512);
	CHECK(p.max_bytes == 5000 && p.max_big == 1 && p.max_slots == 512);
}

int main()
{
	std::mt19937_64 rng(20261018);
	for (Kind k : {INSERT, SERIAL, CLASSIFY, CAPPED})
		random_cases(k, 3000, rng);
	edges();
	gpu_case();
	printf("mibf plan test passed: %llu cases\n", g_case);
	return 0;
}
