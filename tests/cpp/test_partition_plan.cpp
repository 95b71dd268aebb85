// tests/cpp/test_partition_plan.cpp -- the batch planner of the partitioned pipeline (csrc/part_plan.hpp) over a grid of
// probe counts, budgets and geometries, against byte accounting and a brute-force search written here a second time.
// Stand-alone: the header alone, no HIP.  tests/test_partition_plan_cpu.py builds it with -fsanitize=address,undefined.
#include "../../btl_bloomfilter_amd/csrc/part_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace btlbf;

static int g_failed = 0;
#define CHECK(cond, ...)                                   \
	do {                                                   \
		if (!(cond)) {                                     \
			++g_failed;                                    \
			std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
			std::printf(__VA_ARGS__);                      \
			std::printf("\n");                             \
		}                                                  \
	} while (0)

// ---- the rules once more, from DESIGN.md section 4.3, in this file's own words --------------------------------------
static uint64_t my_chunks(double mean, uint32_t epc)
{
	const double m = mean + 8.0 * std::sqrt(mean + 1.0) + 32.0;
	return (uint64_t)std::ceil(m / epc) + 1;
}
static uint64_t my_level(double entries, double useful, uint64_t alloc, uint64_t regions, uint32_t epc)
{
	return (alloc * regions * 4 + 255) / 256 * 256 + alloc * regions * my_chunks(entries / (useful * regions), epc) * 128;
}
static double my_entries(const CarryGeom& g, uint64_t tiles)
{
	return (double)((tiles + g.regions0 - 1) / g.regions0 * g.regions0) * g.probes_per_tile;
}
static uint64_t my_batch(const CarryGeom& g, uint64_t tiles)
{
	return g.extra_bytes + my_level(my_entries(g, tiles), g.bins0, g.bins0, g.regions0, 32) +
	       my_level(my_entries(g, tiles), (double)g.useful1, g.group_bins1, g.regions_group, g.epc1);
}
// bytes in use while phase j of (K, tc) runs: the level-0 buffer (sized for the largest phase), the blocks written so far
// and the one being written, all K blocks' counts, and in the final phase the group buffer
static uint64_t my_phase(const CarryGeom& g, uint32_t K, uint64_t tc, uint32_t j)
{
	const uint64_t tf = g.n_tiles - K * tc;
	const uint64_t l0 = my_level(my_entries(g, std::max(tc, tf)), g.bins0, g.bins0, g.regions0, 32);
	const uint64_t block_ent = g.bins1 * g.regions_carry * my_chunks(my_entries(g, tc) / ((double)g.useful1 * g.regions_carry), g.epc1) * 128;
	const uint64_t cnts = (K * g.bins1 * g.regions_carry * 4 + 255) / 256 * 256;
	const uint64_t group = my_level(my_entries(g, tf), (double)g.useful1, g.group_bins1, g.regions_group, g.epc1);
	return g.extra_bytes + l0 + cnts + std::min<uint64_t>(j + 1, K) * block_ent + (j >= K ? group : 0);
}
static uint64_t my_peak(const CarryGeom& g, uint32_t K, uint64_t tc)
{
	uint64_t peak = 0;
	for (uint32_t j = 0; j <= K; ++j)
		peak = std::max(peak, my_phase(g, K, tc, j));
	return peak;
}
// is any carried size feasible for K?  Every size where the tiles are few, else 512 sizes evenly spread.
static bool my_feasible(const CarryGeom& g, uint32_t K, uint64_t budget)
{
	// (pass C walks up to 16 regions per segment one by one and keeps a table of up to 1024: a plan stays on its side)
	if (g.regions_group + (uint64_t)K * g.regions_carry > (g.regions_group <= 16 ? 16u : 1024u) || g.n_tiles < K + 1)
		return false;
	const uint64_t hi = (g.n_tiles - 1) / K;
	if (hi <= 4096) {
		for (uint64_t tc = 1; tc <= hi; ++tc)
			if (my_peak(g, K, tc) <= budget)
				return true;
		return false;
	}
	for (uint32_t i = 1; i <= 512; ++i) {
		const uint64_t tc = (uint64_t)((unsigned __int128)hi * i / 512);
		if (tc && my_peak(g, K, tc) <= budget)
			return true;
	}
	return false;
}

// ---- geometries ----------------------------------------------------------------------------------------------------
struct Geo {
	const char* name;
	uint32_t bins0, regions_group, regions_carry, epc1;
	uint64_t bins1, useful1, group_bins1;
};
static const Geo kGeos[] = {
    // C2: 2^39 bits, 2^19 segments of 128 KiB as 512 bins x 1024 ways, packed, groups of 64 bins
    {"C2", 512, 8, 1, 48, 1ull << 19, 1ull << 19, 64ull * 1024},
    // 3 x 2^37 bits: 393216 segments as 512 bins of 768 whole segments, packed
    {"3x2^37", 512, 8, 1, 48, 512ull * 768, 393216, 64ull * 768},
    // 2^18 segments as 256 bins x 1024 ways: the groups of 32 bins are written by 16 slices, so no block may join them
    {"2^18 256x1024", 256, 16, 2, 48, 1ull << 18, 1ull << 18, 32ull * 1024},
    // a counting filter of 2^34 counters: 2^18 segments as 512 x 512, 32-bit entries
    {"counting", 512, 8, 1, 32, 1ull << 18, 1ull << 18, 64ull * 512},
    // a small filter: 64 bins x 64 ways, groups of 8 bins written by 64 slices -- pass C walks by its region table
    {"2^31", 64, 64, 8, 32, 4096, 4096, 8 * 64},
};

static CarryGeom make(const Geo& q, double probes, uint64_t budget)
{
	CarryGeom g;
	g.probes_per_tile = 68.0 * 120 * 4 + 1; // 68 reads of 150 bp per tile, k = 31, h = 4
	g.n_tiles = std::max<uint64_t>(1, (uint64_t)(probes / g.probes_per_tile));
	g.regions0 = 256;
	g.bins0 = q.bins0;
	g.bins1 = q.bins1;
	g.useful1 = q.useful1;
	g.group_bins1 = q.group_bins1;
	g.regions_group = q.regions_group;
	g.regions_carry = q.regions_carry;
	g.epc1 = q.epc1;
	const bool full = budget >= (2ull << 30);
	const uint64_t fail_cap = full ? 4ull << 20 : 256ull << 10, spill_cap = full ? 16ull << 20 : 512ull << 10;
	const uint64_t tail = std::max<uint64_t>(256 + fail_cap * 24, 256 + spill_cap * 8);
	g.extra_bytes = (tail + 255) / 256 * 256 + (full ? 256ull * 2 * 32768 * 4 : 0);
	return g;
}

static void check_one(const Geo& q, double probes, uint64_t budget, int& n_carried, int& n_legacy_multi)
{
	const CarryGeom g = make(q, probes, budget);
	const CarryPlan p = plan_call(g, budget);
	const CarryPlan old = plan_call(g, budget, false);
	// the independent batches, by this file's accounting: they fit, and one tile more per batch would not be proposed
	if (old.tiles_per_batch) {
		CHECK(my_batch(g, old.tiles_per_batch) <= budget, "%s %g %llu", q.name, probes, (unsigned long long)budget);
		CHECK(old.bytes_total == my_batch(g, old.tiles_per_batch), "%s: legacy bytes", q.name);
	} else {
		CHECK(my_batch(g, 1) > budget, "%s: one tile fits but nothing was planned", q.name);
	}
	if (p.K == 0) {
		// the plan of old, field by field
		CHECK(p.tiles_per_batch == old.tiles_per_batch && p.bytes_total == old.bytes_total && p.l0.cap == old.l0.cap &&
		          p.group.cap == old.group.cap && p.tiles_carried == 0,
		      "%s: K = 0 differs from the independent batches", q.name);
		if (old.tiles_per_batch && old.tiles_per_batch < g.n_tiles) {
			++n_legacy_multi;
			for (uint32_t K = 1; K <= kCarryMaxBatches; ++K)
				CHECK(!my_feasible(g, K, budget), "%s %g %llu: K = %u fits, independent batches planned", q.name, probes,
				      (unsigned long long)budget, K);
		}
		return;
	}
	++n_carried;
	CHECK(old.tiles_per_batch && old.tiles_per_batch < g.n_tiles, "%s: carried although one batch suffices", q.name);
	CHECK(p.K <= kCarryMaxBatches && q.regions_group + p.K * q.regions_carry <= (q.regions_group <= 16 ? 16u : 1024u), "%s: K = %u", q.name, p.K);
	// the phases: every tile once and in order, each phase within the budget
	uint64_t next = 0;
	for (uint32_t j = 0; j <= p.K; ++j) {
		CHECK(p.phase_first(j) == next && p.phase_tiles(j, g.n_tiles) >= 1, "%s: phase %u", q.name, j);
		next += p.phase_tiles(j, g.n_tiles);
		CHECK(p.phase_bytes(j, g) <= budget, "%s: phase %u over the budget", q.name, j);
		CHECK(p.phase_bytes(j, g) == my_phase(g, p.K, p.tiles_carried, j), "%s: phase %u bytes %llu, recomputed %llu", q.name, j,
		      (unsigned long long)p.phase_bytes(j, g), (unsigned long long)my_phase(g, p.K, p.tiles_carried, j));
	}
	CHECK(next == g.n_tiles, "%s: the phases cover %llu of %llu tiles", q.name, (unsigned long long)next, (unsigned long long)g.n_tiles);
	CHECK(p.bytes_total == my_peak(g, p.K, p.tiles_carried) && p.bytes_total <= budget, "%s: peak", q.name);
	for (uint32_t K = 1; K < p.K; ++K)
		CHECK(!my_feasible(g, K, budget), "%s %g %llu: K = %u fits, K = %u planned", q.name, probes, (unsigned long long)budget, K, p.K);
}

int main()
{
	const double probes[] = {1e6, 3.3e6, 1e7, 1e8, 1.44e8, 1e9, 4.8e9, 1.6e10, 4.8e10, 5e10};
	const uint64_t budgets[] = {1ull << 20,  24ull << 20, 64ull << 20,  200ull << 20,       1ull << 30,         3ull << 30,  16ull << 30,
	                            40ull << 30, 100ull << 30, 171000000000ull, 180000000000ull, 230000000000ull};
	int n_carried = 0, n_legacy_multi = 0, n = 0;
	for (const Geo& q : kGeos)
		for (double pr : probes)
			for (uint64_t b : budgets) {
				check_one(q, pr, b, n_carried, n_legacy_multi);
				++n;
			}
	// budgets a little below what one batch takes: where a carried plan is the answer, if the geometry allows one
	for (const Geo& q : kGeos)
		for (double pr : probes)
			for (double share : {0.97, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3}) {
				const uint64_t b = (uint64_t)(share * (double)my_batch(make(q, pr, 4ull << 30), make(q, pr, 4ull << 30).n_tiles));
				check_one(q, pr, b, n_carried, n_legacy_multi);
				++n;
			}
	CHECK(n_carried >= 40 && n_legacy_multi >= 50, "the grid exercises %d carried and %d multi-batch legacy plans", n_carried, n_legacy_multi);
	// C2 as the benchmark runs it: one sweep at either estimate of the budget, no plan change with room for one batch
	for (uint64_t b : {171000000000ull, 180000000000ull}) {
		const CarryGeom g = make(kGeos[0], 4.8e10, b);
		const CarryPlan p = plan_call(g, b);
		CHECK(p.K >= 1 && p.K <= 2, "C2 at %llu bytes: K = %u", (unsigned long long)b, p.K);
		std::printf("C2 budget %.1f GB: one batch %.1f GB, K = %u, carried %.1f %% each, peak %.1f GB\n", b / 1e9, my_batch(g, g.n_tiles) / 1e9,
		            p.K, 100.0 * p.tiles_carried / g.n_tiles, p.bytes_total / 1e9);
	}
	{
		const CarryGeom g = make(kGeos[0], 4.8e10, 230000000000ull);
		const CarryPlan p = plan_call(g, 230000000000ull);
		CHECK(p.K == 0 && p.tiles_per_batch == g.n_tiles, "C2 fits one batch of 230 GB");
	}
	std::printf("%d plans, %d carried, %d multi-batch legacy\n", n, n_carried, n_legacy_multi);
	if (g_failed) {
		std::printf("%d checks failed\n", g_failed);
		return 1;
	}
	std::printf("partition plan test passed\n");
	return 0;
}
