// csrc/part_plan.hpp -- how the tiles of one partitioned call are cut into batches under the scratch budget.  Plain
// integers and host arithmetic only (no HIP header): tests/cpp/test_partition_plan.cpp includes it alone.
//
// A call whose scratch does not fit the budget used to run as independent batches, each with its own pass C over the
// whole array.  A CARRIED plan runs K carried batches and one final batch instead: a carried
// batch is taken through pass A and one ungrouped pass B, and its segment regions are kept as one BLOCK; the final batch
// runs group by group as ever, and its pass C walks the group buffer's regions and the K carried regions of every
// segment -- one sweep of the array per call.  The carried batches are equal in size, so the blocks are the origin
// blocks of one PartIn.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace btlbf {

static constexpr uint32_t kPlanChunkBytes = 128; // one chunk (internal.hpp kChunk words)
static constexpr uint32_t kCarryMaxBatches = 4;  // K is looked for up to here
static constexpr uint32_t kCarryMaxRegions = 16; // regions per segment pass C walks one by one (kApplyFewRegions)
static constexpr uint32_t kCarryMaxTabled = 1024; // regions per segment pass C keeps a table of (kApplyMaxRegions)
static constexpr uint32_t kCarryGrid = 4096;     // sizes of a carried batch that are tried: i / kCarryGrid of 1/K of the call

// chunks a region needs for `mean_entries` expected entries (Poisson: mean + 8 sigma) plus the
// partially filled chunk flushed at kernel end
// (chunks of `epc` entries: kChunk, or kPackChunk on a packed level)
inline uint32_t chunks_for(double mean_entries, uint32_t tail_chunks, uint32_t epc)
{
	const double m = mean_entries + 8.0 * std::sqrt(mean_entries + 1.0) + 32.0;
	return (uint32_t)std::min<double>(4.0e9, std::ceil(m / (double)epc)) + tail_chunks;
}

// pass A gives every workgroup (= region) ceil(tiles / regions) tiles: capacities are planned for the
// fullest region, which matters when a batch has only a few tiles per workgroup
inline uint64_t tiles_for_caps(uint64_t tiles, uint32_t regions)
{
	return regions ? (tiles + regions - 1) / regions * regions : tiles;
}

// the arrays of one level: `alloc_bins` bins of `regions` regions, sized for `entries` spread over `useful_bins` bins
struct LevelBytes {
	uint32_t cap = 0; // chunks per region
	uint64_t cnt_bytes = 0, ent_bytes = 0;
	uint64_t bytes() const { return cnt_bytes + ent_bytes; }
};
inline LevelBytes level_bytes(double entries, double useful_bins, uint64_t alloc_bins, uint32_t regions, uint32_t epc)
{
	LevelBytes b;
	b.cap = chunks_for(entries / (useful_bins * regions), 1, epc);
	b.cnt_bytes = (alloc_bins * regions * 4 + 255) / 256 * 256;
	b.ent_bytes = alloc_bins * regions * b.cap * kPlanChunkBytes;
	return b;
}

// The independent batches of old: the largest batch, in tiles, whose bytes fit the budget (bytes_of(tiles) says what a
// batch takes); 0 = not even one tile fits.
template <class F>
inline uint64_t batch_tiles_for_budget(uint64_t n_tiles, uint64_t budget, F bytes_of)
{
	uint64_t tiles = n_tiles;
	for (int iter = 0; iter < 64; ++iter) {
		const uint64_t bytes = bytes_of(tiles);
		if (bytes <= budget || tiles <= 1)
			break;
		const double ratio = (double)budget / (double)bytes;
		const uint64_t nt = (uint64_t)((double)tiles * ratio * 0.95);
		tiles = nt >= tiles ? tiles - 1 : (nt ? nt : 1);
	}
	return bytes_of(tiles) <= budget ? tiles : 0;
}

// what the planner needs to know of a one-split plan (pass A -> level-0 bins -> one pass B -> segments)
struct CarryGeom {
	uint64_t n_tiles = 0;        // pass-A tiles of the call
	double probes_per_tile = 0;  // expected entries of one tile
	uint32_t regions0 = 0;       // pass-A workgroups = regions per level-0 bin
	uint32_t bins0 = 0;          // level-0 bins
	uint64_t bins1 = 0;          // the split level's bins over the whole array ...
	uint64_t useful1 = 0;        // ... of which this many are segments of the array
	uint64_t group_bins1 = 0;    // bins of it the group buffer holds
	uint32_t regions_group = 0;  // writers per bin of the group buffer
	uint32_t regions_carry = 0;  // writers per bin of a carried block (pass B over all level-0 bins at once)
	uint32_t epc1 = 32;          // entries per chunk of the split level (packed or not)
	uint64_t extra_bytes = 0;    // the tail (fail / spill lists) and pass A's late images
};

struct CarryPlan {
	uint32_t K = 0;                  // carried batches; 0 = independent batches of tiles_per_batch tiles
	uint64_t tiles_per_batch = 0;    // K == 0: tiles of an independent batch (0: nothing fits)
	uint64_t tiles_carried = 0;      // K >= 1: tiles of each carried batch; the final batch takes the rest
	LevelBytes l0, group, block;     // the level-0 buffer (largest phase), the group buffer, ONE carried block
	uint64_t carry_cnt_bytes = 0;    // the K blocks' counts, contiguous and padded once
	uint64_t bytes_total = 0;        // the scratch: the peak over the phases (= the final phase)
	uint64_t tiles_final(uint64_t n_tiles) const { return n_tiles - K * tiles_carried; }
	// phase j < K: carried batch j; phase K: the final batch
	uint64_t phase_first(uint32_t j) const { return (uint64_t)j * tiles_carried; }
	uint64_t phase_tiles(uint32_t j, uint64_t n_tiles) const { return j < K ? tiles_carried : tiles_final(n_tiles); }
	uint64_t phase_bytes(uint32_t j, const CarryGeom& g) const
	{ // blocks written so far and the one being written, the level-0 buffer; the final phase: all blocks + the group buffer
		const uint64_t blocks = std::min<uint64_t>(j + 1, K);
		return g.extra_bytes + l0.bytes() + carry_cnt_bytes + blocks * block.ent_bytes + (j >= K ? group.bytes() : 0);
	}
};

inline double carry_entries(const CarryGeom& g, uint64_t tiles)
{
	return (double)tiles_for_caps(tiles, g.regions0) * g.probes_per_tile;
}

// bytes of one independent batch of `tiles` tiles
inline uint64_t legacy_bytes(const CarryGeom& g, uint64_t tiles, LevelBytes* l0 = nullptr, LevelBytes* group = nullptr)
{
	const double e = carry_entries(g, tiles);
	const LevelBytes a = level_bytes(e, (double)g.bins0, g.bins0, g.regions0, kPlanChunkBytes / 4);
	const LevelBytes b = level_bytes(e, (double)g.useful1, g.group_bins1, g.regions_group, g.epc1);
	if (l0)
		*l0 = a;
	if (group)
		*group = b;
	return a.bytes() + b.bytes() + g.extra_bytes;
}

// K carried batches of tc tiles each and a final batch of the rest (at least one tile): the exact bytes
inline CarryPlan carry_eval(const CarryGeom& g, uint32_t K, uint64_t tc)
{
	CarryPlan p;
	p.K = K;
	p.tiles_carried = tc;
	const uint64_t tf = g.n_tiles - K * tc;
	p.l0 = level_bytes(carry_entries(g, std::max(tc, tf)), (double)g.bins0, g.bins0, g.regions0, kPlanChunkBytes / 4);
	p.group = level_bytes(carry_entries(g, tf), (double)g.useful1, g.group_bins1, g.regions_group, g.epc1);
	p.block = level_bytes(carry_entries(g, tc), (double)g.useful1, g.bins1, g.regions_carry, g.epc1);
	p.carry_cnt_bytes = (K * g.bins1 * g.regions_carry * 4 + 255) / 256 * 256;
	p.bytes_total = p.phase_bytes(K, g);
	return p;
}

inline bool carry_allowed(const CarryGeom& g, uint32_t K)
{
	// pass C stays on the walk it is on: one by one where the group buffer alone has few regions per segment (the large
	// filters), by the region table otherwise
	const uint64_t most = g.regions_group <= kCarryMaxRegions ? kCarryMaxRegions : kCarryMaxTabled;
	return g.regions_carry >= 1 && (uint64_t)g.regions_group + (uint64_t)K * g.regions_carry <= most && g.n_tiles >= K + 1;
}

// the carried batch sizes that are tried for K: i / kCarryGrid of n_tiles / K, every size where there are few tiles
inline uint64_t carry_candidate(const CarryGeom& g, uint32_t K, uint32_t i)
{
	const uint64_t hi = (g.n_tiles - 1) / K; // the final batch keeps a tile
	if (hi <= kCarryGrid)
		return i >= 1 && i <= hi ? i : 0;
	return (uint64_t)((unsigned __int128)hi * i / kCarryGrid);
}

// The plan of a call: one batch if it fits; else the smallest K >= 1 for which some carried size fits the budget in
// every phase (of those sizes the one with the smallest peak); else independent batches as of old.  carry == false
// (BTLBF_CARRY=0) keeps the independent batches.
inline CarryPlan plan_call(const CarryGeom& g, uint64_t budget, bool carry = true)
{
	CarryPlan legacy;
	legacy.tiles_per_batch = batch_tiles_for_budget(g.n_tiles, budget, [&](uint64_t t) { return legacy_bytes(g, t); });
	if (legacy.tiles_per_batch)
		legacy.bytes_total = legacy_bytes(g, legacy.tiles_per_batch, &legacy.l0, &legacy.group);
	if (!carry || legacy.tiles_per_batch == 0 || legacy.tiles_per_batch >= g.n_tiles)
		return legacy;
	for (uint32_t K = 1; K <= kCarryMaxBatches && carry_allowed(g, K); ++K) {
		CarryPlan best;
		for (uint32_t i = 1; i <= kCarryGrid; ++i) {
			const uint64_t tc = carry_candidate(g, K, i);
			if (tc == 0)
				continue;
			const CarryPlan p = carry_eval(g, K, tc);
			if (p.bytes_total <= budget && (best.K == 0 || p.bytes_total < best.bytes_total))
				best = p;
		}
		if (best.K)
			return best;
	}
	return legacy;
}

// K equal carried batches whether or not one batch would fit (BTLBF_CARRY_FORCE, for tests: small calls then take the
// carried form); K == 0 in the result: the geometry, the tile count or the budget does not allow it
inline CarryPlan plan_forced(const CarryGeom& g, uint64_t budget, uint32_t K)
{
	if (K < 1 || K > kCarryMaxBatches || !carry_allowed(g, K))
		return CarryPlan();
	const CarryPlan p = carry_eval(g, K, g.n_tiles / (K + 1));
	return p.bytes_total <= budget ? p : CarryPlan();
}

} // namespace btlbf
