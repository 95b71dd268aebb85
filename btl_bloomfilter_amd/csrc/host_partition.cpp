// csrc/host_partition.cpp -- the partitioned pipeline on the host side: planning (segments, levels, caps, scratch),
// the partitioned insert and query, and the multi-GPU routing entry points over the same planner.
//
// A call plans once and passes the plan down: part_prepare (PartPrep) for the single-GPU pipeline -- the SplitCold
// route of a query hands it the level-0 plan it has already made --, plan_routed (RoutePlan) for the routing entry
// points.  The fail-list constants, the named rules and every plan_* function are private to this unit, except what
// the query routing (host_query.cpp) decides and executes with: that is declared in host_partition.hpp, which only
// these two units include.  The sequence path (host_seq.cpp) enters through want_partitioned and partitioned_insert
// (host_internal.hpp) and, for queries, through host_query.cpp's contains_routed.  The scratch lives in the filter's
// DevScratch buffers.  Kernels: partition_kernels.hip, part_hash_inst.hip.  How a call is cut into batches under the
// scratch budget -- one batch, carried batches with one pass C, or independent batches -- is part_plan.hpp's arithmetic.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"
#include "host_partition.hpp"
#include "part_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace btlbf;

namespace {

// partitioned query: room for the failed positions of one batch and their hash set
static constexpr uint64_t kFailCap = 4ull << 20;          // entries
static constexpr uint64_t kFailTableSlots = 2 * kFailCap; // power of two
// entries a FRESH insert batch (partitioned_insert) may report as explicit positions instead of staging them
static constexpr uint64_t kFreshSpillCap = 16ull << 20;

// (chunks_for, tiles_for_caps, level_bytes: part_plan.hpp, the byte arithmetic of every plan made here)
static_assert(kPlanChunkBytes == kChunk * 4, "part_plan.hpp counts chunks of kChunk words");

unsigned ceil_log2(uint64_t x)
{
	unsigned b = 0;
	while ((1ull << b) < x)
		++b;
	return b;
}

// mloc = positions held locally; unit_shift = log2(positions per byte): 3 for bits, 0 for uint8_t counters
bool plan_segments(uint64_t mloc, PartPlan& pl, uint32_t unit_shift = 3)
{
	// 64 KiB segments (two pass-C workgroups per CU) as long as they number at most 2^19, else 128 KiB:
	// with more than 512 x 1024 segments pass A would need 1024 level-0 bins, whose 32-entry rings make
	// a quarter of the entries take the late path (measured: pass A 63 -> 54 ms at 512 bins; the
	// read-only pass C loses 0.7 ms per launch with one workgroup per CU)
	const uint32_t small = 16 + unit_shift;
	pl.counting = unit_shift == 0;
	pl.seg_shift = small;
	if (((mloc + (1ull << small) - 1) >> small) > 512ull * 1024)
		pl.seg_shift = small + 1;
	pl.n_seg = (mloc + (1ull << pl.seg_shift) - 1) >> pl.seg_shift;
	// up to 2^20 segments: pass A x one split pass; up to 2^22 (a 256 GiB bit array and beyond): two split passes
	// (entries stay 32-bit: 1024 level-0 bins of at most 2^32 positions)
	return pl.n_seg <= 4096ull * 1024;
}

// Slices of a split pass: workgroup (bin, slice) of bins_g input bins, each slice taking every `slices`-th input
// region of its bin (at most r_in).  About two workgroups per CU, but a whole number of rounds over the CUs: with
// 48 bins per group (a 3 x 2^37-bit filter) the old rule, ceil(512 / bins), gave 528 workgroups -- two full rounds of
// 256 and a third for 16 of them, and the split pass took 5.8 ms instead of 4.2.  Looked for between half of that rule's
// count and 16 (pass C walks up to 16 regions per segment one by one, kApplyFewRegions) or the rule's count if larger.
uint32_t split_slices(uint32_t bins_g, uint32_t r_in, uint32_t cus)
{
	const uint32_t want = std::max(1u, std::min(r_in, (2 * cus + bins_g - 1) / bins_g)); // the old rule
	const uint32_t hi = std::max(1u, std::min(r_in, std::max(want, 16u)));
	uint32_t best = want;
	double best_cost = 1e30;
	for (uint32_t s = std::max(1u, want / 2); s <= hi; ++s) {
		const uint64_t wg = (uint64_t)bins_g * s;
		const double rounds = (double)((wg + cus - 1) / cus);
		// time ~ rounds x work per workgroup; a slight preference for the grid the rule aimed at
		const double cost = rounds / (double)wg * (1.0 + 0.02 * std::abs((double)s - (double)want) / (double)want);
		if (cost < best_cost) {
			best_cost = cost;
			best = s;
		}
	}
	return best;
}

// append the split levels that take bins of 2^lv[0].shift positions down to segments
bool plan_splits(PartPlan& pl, uint32_t regions_in_total, uint32_t cus = 256)
{
	pl.n_levels = 1;
	uint32_t regions_in = regions_in_total;
	if (pl.lv[0].wseg) { // bins of wseg segments: one split pass, wseg ways, straight to (real) segment numbers
		PartLevel& o = pl.lv[1];
		o.P = pl.lv[0].wseg;
		o.bins = pl.lv[0].bins * o.P;
		o.shift = pl.seg_shift;
		o.regions = split_slices(pl.lv[0].bins, regions_in, cus);
		pl.n_levels = 2;
	} else {
		const uint32_t rb = pl.lv[0].shift - pl.seg_shift;
		if (rb == 0)
			return true;
		if (rb > 20)
			return false;
		const uint32_t fan[2] = {rb <= 10 ? rb : rb - rb / 2, rb <= 10 ? 0 : rb / 2};
		for (int j = 0; j < 2 && fan[j]; ++j) {
			PartLevel& in = pl.lv[pl.n_levels - 1];
			PartLevel& o = pl.lv[pl.n_levels];
			o.P = 1u << fan[j];
			o.bins = in.bins * o.P;
			o.shift = in.shift - fan[j];
			o.regions = split_slices(in.bins, regions_in, cus);
			regions_in = o.regions;
			++pl.n_levels;
		}
	}
	// the split levels and the apply pass run in groups of level-0 bins (split a group all the way
	// down, apply its segments, next group): the arrays of the split levels then hold one group
	// instead of the whole batch, so a batch can be almost twice as large for the same scratch and the
	// filter is swept fewer times
	pl.group_bins = 0;
	if (pl.n_levels >= 2 && pl.lv[0].bins >= 16) {
		pl.group_bins = (pl.lv[0].bins + 7) / 8;
		uint32_t bins_g = pl.group_bins, r_in = regions_in_total;
		for (int j = 1; j < pl.n_levels; ++j) {
			pl.lv[j].regions = split_slices(bins_g, r_in, cus);
			r_in = pl.lv[j].regions;
			bins_g *= pl.lv[j].P;
		}
	}
	return true;
}

// tuning knob: BTLBF_PACKED=0 keeps every level on 32-bit entries
bool packed_enabled()
{
	const char* e = getenv("BTLBF_PACKED");
	return !(e && e[0] == '0');
}

// tuning knob: BTLBF_CARRY=0 keeps the independent batches where a call does not fit one (read at plan time)
bool carry_enabled()
{
	const char* e = getenv("BTLBF_CARRY");
	return !(e && e[0] == '0');
}

// BTLBF_CARRY_FORCE=K (1 .. kCarryMaxBatches) exists for tests: K equal carried batches even where one batch would fit,
// so that small calls exercise the carried form
uint32_t carry_forced()
{
	const char* e = getenv("BTLBF_CARRY_FORCE");
	const int v = e ? atoi(e) : 0;
	return v >= 1 && v <= (int)kCarryMaxBatches ? (uint32_t)v : 0;
}

// capacities + byte sizes for `entries` expected entries in the whole batch
void plan_caps(PartPlan& pl, double entries, int first_level)
{
	pl.bytes_total = 0;
	for (int j = first_level; j < pl.n_levels; ++j) {
		PartLevel& l = pl.lv[j];
		// the last level has n_seg useful bins although bins may be rounded up
		const double useful = j == pl.n_levels - 1 ? (double)std::min<uint64_t>(pl.n_seg, l.bins) : (double)l.bins;
		// The format of the level, decided here and nowhere else: the LAST split level writes packed chunks -- 48
		// entries per 128-byte line instead of 32 -- when its rings hold one chunk and its entries fit 20 bits
		// (part_packs); pass A's output, other split levels and counting filters keep 32-bit entries.
		// BTLBF_PACKED=0 (tuning knob, read at plan time like BTLBF_SPLIT_BITS) keeps every level on 32-bit entries.
		l.packed = j >= 1 && j == pl.n_levels - 1 && !pl.counting && part_packs(l.P, l.shift) && packed_enabled();
		l.alloc_bins = l.bins;
		if (j >= 1 && pl.group_bins) {
			l.alloc_bins = pl.group_bins;
			for (int i = 1; i <= j; ++i)
				l.alloc_bins *= pl.lv[i].P;
		}
		const LevelBytes lb = level_bytes(entries, useful, l.alloc_bins, l.regions, part_epc(l.packed));
		l.cap = lb.cap;
		l.cnt_bytes = lb.cnt_bytes;
		l.ent_bytes = lb.ent_bytes;
		pl.bytes_total += l.cnt_bytes + l.ent_bytes;
	}
}

uint8_t* carve_levels(PartPlan& pl, uint8_t* p, int first_level)
{
	for (int j = first_level; j < pl.n_levels; ++j) {
		pl.lv[j].cnt = reinterpret_cast<uint32_t*>(p);
		p += pl.lv[j].cnt_bytes;
		pl.lv[j].ent = reinterpret_cast<uint32_t*>(p);
		p += pl.lv[j].ent_bytes;
	}
	return p;
}

unsigned cu_count(int device)
{
	int cus = 256;
	(void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
	return (unsigned)cus;
}

// expected probes of one full pass-A tile (+1 so that capacities never come out as zero)
double probes_per_tile(const btlbf_filter* f, const PartTiling& tl)
{
	return tl.windows_per_tile * f->hp.h + 1.0;
}

// The side block of a pass over f's array: what the filter fixes (bits or counters, the threshold of a counting query,
// the base of the positions a pass reports) and, for a pass A planned here, its late images and how level-0 bins map
// to positions (PartSide::bin_wseg).  The fail, spill and fresh fields are the caller's.
PartSide part_side(const btlbf_filter* f, const PartPlan* pl = nullptr)
{
	PartSide sd;
	memset(&sd, 0, sizeof sd);
	sd.pos_base = f->mod.shard_lo;
	sd.counting = f->kind == BTLBF_COUNTING8;
	sd.threshold = f->thr;
	if (pl) {
		sd.late_buf = pl->late_buf;
		sd.late_cap = pl->late_cap;
		sd.bin_wseg = pl->lv[0].wseg;
		sd.bin_magic = pl->lv[0].wseg ? (uint32_t)(((1ull << 32) + pl->lv[0].wseg - 1) / pl->lv[0].wseg) : 0;
		sd.bin_seg_shift = pl->seg_shift;
		sd.bin_width = pl->lv[0].wseg << pl->seg_shift;
	}
	return sd;
}

// run the split levels lv[1..] over the level-0 data `in0`, then the apply / test pass
// in0 holds level-0 bins [bin_offset, bin_offset + n_bins0) of the local array (bin i of in0 = absolute bin
// bin_offset + i); the whole array by default
// `carried`: the blocks earlier batches of the call left (run_unit), which pass C walks behind each group's own regions
int run_levels(btlbf_filter* f, PartPlan& pl, PartIn in0, const PartSide& sd, int query, hipStream_t s,
               uint32_t bin_offset = 0, uint32_t n_bins0 = 0, const PartIn* carried = nullptr)
{
	const int exact = sd.counting && !query; // counter increments: every entry exactly once
	if (f->lazy_zero && !(sd.fresh && !query)) // only a fresh insert may run on a lazily cleared array
		return fail(BTLBF_EINVAL, "internal error: partition passes on a lazily cleared array");
	const int prof_split = query ? BTLBF_PROF_QUERY_SPLIT : BTLBF_PROF_INSERT_SPLIT;
	const int prof_apply = query ? BTLBF_PROF_QUERY_TEST : BTLBF_PROF_INSERT_APPLY;
	if (n_bins0 == 0)
		n_bins0 = pl.lv[0].bins - bin_offset;
	// group by group: split the group's level-0 bins all the way down, then apply its segments
	// (plans without groups: one group of everything)
	const uint32_t group = pl.group(n_bins0);
	for (uint32_t b0 = 0; b0 < n_bins0; b0 += group) {
		PartIn in = in0;
		uint32_t first_in = b0, abs_first = bin_offset + b0, n_in = std::min(group, n_bins0 - b0);
		uint32_t in_shift = pl.lv[0].shift;
		for (int j = 1; j < pl.n_levels; ++j) {
			ProfSpan ps(f, prof_split, s);
			HIP_TRY(launch_part_split(f->d_data, in, first_in, abs_first, n_in, pl.lv[j].out(), pl.lv[j].shift,
			                          in_shift, sd, query, exact, s));
			in = pl.lv[j].in();
			first_in = 0;
			abs_first *= pl.lv[j].P;
			n_in *= pl.lv[j].P;
			in_shift = pl.lv[j].shift;
		}
		const uint64_t seg_first = abs_first;
		if (seg_first >= pl.n_seg)
			break;
		const uint64_t n_seg = std::min<uint64_t>(n_in, pl.n_seg - seg_first);
		ProfSpan ps(f, prof_apply, s);
		HIP_TRY(launch_part_apply(f->d_data, f->local_bytes, pl.seg_shift, seg_first, n_seg, in, sd, query, s, f->part.p,
		                          carried));
	}
	return BTLBF_OK;
}

// A UNIT of a call: the tiles that reach one pass C -- one of the independent batches, or under a carried plan the
// whole call.
struct PartUnit {
	uint64_t first = 0, n = 0;
};
PartUnit part_unit(const PartPlan& pl, uint64_t total_tiles, uint64_t t0)
{
	if (pl.carry_k)
		return PartUnit{0, total_tiles};
	return PartUnit{t0, std::min<uint64_t>(pl.tiles_per_batch, total_tiles - t0)};
}

// The passes of a unit up to and including its pass C.  Carried plan: carried batch j is hashed and split, all level-0
// bins at once, into block j of pl.carry (absolute segment numbers); the final batch runs group by group, its pass C
// taking the blocks along.  `a`: the call's arguments with the outputs pass A writes; the tile range is set here.
int run_unit(btlbf_filter* f, PartPlan& pl, SeqArgs a, const PartUnit& u, const PartSide& sd, int query, hipStream_t s)
{
	const int exact = sd.counting && !query;
	const uint32_t k = pl.carry_k;
	const PartIn carried = pl.carry_in();
	for (uint32_t j = 0; j <= k; ++j) {
		a.first_tile = u.first + j * pl.carry_tiles;
		a.n_tiles = j < k ? pl.carry_tiles : u.n - k * pl.carry_tiles;
		{
			ProfSpan ps(f, query ? BTLBF_PROF_QUERY_HASH : BTLBF_PROF_INSERT_HASH, s);
			HIP_TRY(launch_part_hash(a, pl.lv[0].out(), pl.lv[0].shift, sd, query, s));
		}
		if (j < k) {
			if (f->lazy_zero && !(sd.fresh && !query))
				return fail(BTLBF_EINVAL, "internal error: partition passes on a lazily cleared array");
			ProfSpan ps(f, query ? BTLBF_PROF_QUERY_SPLIT : BTLBF_PROF_INSERT_SPLIT, s);
			HIP_TRY(launch_part_split(f->d_data, pl.lv[0].in(), 0, 0, pl.lv[0].bins, pl.carry_out(j), pl.carry.shift,
			                          pl.lv[0].shift, sd, query, exact, s));
		} else if (int rc = run_levels(f, pl, pl.lv[0].in(), sd, query, s, 0, 0, k ? &carried : nullptr)) {
			return rc;
		}
	}
	return BTLBF_OK;
}

// AUTO's break-even between the direct kernels and a sweep of the array, as probes per byte of the local array.
// Measured on MI355X at 2^39 bits (tools/auto_probe.py): the direct insert costs 24.4 ms per 10^6 reads of 150 bp (21 G
// atomics/s), the partitioned one 26.5 ms + 1.9 ms per 10^6 reads -- equal at 0.82 %; the direct query 9.3 ms per 10^6
// reads (all hits: four gathers per k-mer), the partitioned one 17.3 ms + 1.6 per 10^6 -- equal at 1.57 %.  (Round 2's
// rule was 2 % for both: a batch of 2x10^6 reads was inserted in 48.7 ms instead of 30.4.)
constexpr double kAutoInsertRatio = 0.0095; // (kAutoQueryRatio = 0.0165: host_partition.hpp)
// plan_level0: calls of this many probes or more (4x10^9 k-mers at h = 4) take 256 level-0 bins where 512 are the rule
constexpr double kWideSplitProbes = 1.6e10;

} // namespace

// ---- what the query routing shares (host_partition.hpp) ---------------------------------------------------------
namespace btlbf {

PartTail part_tail(uint64_t budget)
{
	PartTail t;
	const bool full = budget >= (2ull << 30);
	t.fail_cap = full ? kFailCap : 256ull << 10;
	t.spill_cap = full ? kFreshSpillCap : 512ull << 10;
	t.table_slots = 2 * t.fail_cap;
	t.bytes = std::max<uint64_t>(256 + t.fail_cap * 8 + t.table_slots * 8, 256 + t.spill_cap * 8);
	return t;
}

uint64_t scratch_budget(btlbf_filter* f)
{
	if (f->part_budget)
		return f->part_budget;
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess)
		return 0;
	return (uint64_t)((double)(free_b + f->part.bytes) * 0.80);
}

// probes a call over `len` bases sends to this filter's local array (a shard keeps its window's share)
double local_probes(const btlbf_filter* f, uint64_t len)
{
	return (double)len * f->hp.h * ((double)f->mod.shard_len / (double)f->mod.size);
}

// are `probes` worth a sweep of the local array?  `ratio`: AUTO's break-even in probes per byte of it; and the batch
// must be big enough to be worth the five launches of a sweep
bool worth_sweep(const btlbf_filter* f, double probes, double ratio)
{
	return probes >= ratio * (double)f->local_bytes && probes >= 4.0e6;
}

// the direct kernel that answers contains() for this filter
int direct_query_op(const btlbf_filter* f)
{
	return f->kind == BTLBF_COUNTING8 ? OP_CBF_QUERY : f->shard_count != 1 ? OP_BF_CONTAINS_WIN : OP_BF_CONTAINS;
}

// local_probes -- or, with a scratch budget imposed by the caller, what one batch of that budget holds (about 5.5 bytes
// of scratch per probe; 5.3 where the last split level is packed, its arrays holding an eighth of a batch at a time --
// the rule keeps the larger figure for both): the figure plan_level0's batch-size rule goes by
double call_probes(const btlbf_filter* f, uint64_t len)
{
	const double all = local_probes(f, len);
	return f->part_budget ? std::min(all, (double)f->part_budget / 5.5) : all;
}

// the segment size and the level-0 bins (pass A's output) of this filter's local array; false = no partitioned path
// `call_probes`: probes of the whole call (0 = unknown), for the one choice that depends on the batch size
bool plan_level0(const btlbf_filter* f, PartPlan& pl, double call_probes)
{
	if (!plan_segments(f->mod.shard_len, pl, f->kind == BTLBF_COUNTING8 ? 0 : 3))
		return false;
	PartLevel& l0 = pl.lv[0];
	if (pl.n_seg <= 1024) {
		l0.bins = (uint32_t)pl.n_seg;
		l0.shift = pl.seg_shift;
	} else { // split the segment index bits evenly between pass A and pass B
		unsigned b1 = (ceil_log2(pl.n_seg) + 1) / 2; // pass B takes the larger half: pass A gains more from big rings
		// 2^17 < segments <= 2^18 (bit filters of 8 .. 16 GiB): 512 bins and a 512-way split by that rule, or 256 bins
		// and a 1024-way split.  Pass A is 6 % (plain ntHash: 40.2 -> 37.9 ms per 6x10^9 k-mers) to 8.5 % (four spaced
		// seeds: 89.7 -> 82.1) faster on 128-entry rings; the 1024-way split pass costs the same per launch in batches
		// of 6x10^9 k-mers and 0.4 ms more (of 1.8) in batches of 2.4x10^9 (tools/quick_bench.py with BTLBF_SPLIT_BITS,
		// DESIGN.md B.2) -- so for large calls only.
		if (ceil_log2(pl.n_seg) == 18 && call_probes >= kWideSplitProbes)
			b1 = 10;
		if (const char* e = getenv("BTLBF_SPLIT_BITS")) { // tuning knob: segment-index bits left to pass B
			const int v = atoi(e);
			if (v >= 1 && v <= 10 && ceil_log2(pl.n_seg) - v <= 10)
				b1 = (unsigned)v;
		}
		if (ceil_log2(pl.n_seg) > b1 + 10)
			b1 = ceil_log2(pl.n_seg) - 10; // pass A writes at most 1024 bins
		l0.shift = pl.seg_shift + b1;
		l0.bins = (uint32_t)((pl.n_seg + (1ull << b1) - 1) >> b1);
		if (l0.shift > 32)
			return false; // (cannot happen below 2^22 segments)
		// A bin count that is no power of two leaves staging rings of pass A unused while the others take more
		// entries per round than they are sized for: 3 x 2^37 bits gave 384 bins on the 512-ring geometry, a third
		// more entries per ring and round, and pass A took 22.2 ms per 2.4x10^9 k-mers where a filter of 512 bins and the
		// same reduction takes 18.6.  So the bins are made of a whole number of SEGMENTS instead, as many as fill the
		// geometry's rings (768 segments per bin there, 512 bins); pass B then splits wseg ways.  One split level only.
		const uint32_t rings = 1u << ceil_log2(l0.bins);
		if (l0.bins < rings && b1 <= 10) {
			l0.wseg = (uint32_t)((pl.n_seg + rings - 1) / rings);
			l0.bins = (uint32_t)((pl.n_seg + l0.wseg - 1) / l0.wseg);
		}
	}
	l0.P = l0.bins;
	l0.alloc_bins = l0.bins;
	return true;
}

} // namespace btlbf

namespace {

// what part_prepare makes of a buffer
struct PartPrep {
	PartPlan pl;
	PartTiling tiling{};
	PartTail tail{};
	uint8_t* extra = nullptr; // the tail's place in the scratch
	bool ok = false;          // false = not applicable, use the direct kernel
};

// plan the single-GPU pipeline for a buffer and (re)allocate the scratch; `level0`: the caller's plan_level0 of this
// very buffer, where it has made one already (the split query)
PartPrep part_prepare(btlbf_filter* f, const SeqArgs& base, int mode, double auto_ratio, const PartPlan* level0 = nullptr)
{
	PartPrep pp;
	PartPlan& pl = pp.pl;
	if (level0)
		pl = *level0;
	else if (!plan_level0(f, pl, call_probes(f, base.len)))
		return pp;
	PartLevel& l0 = pl.lv[0];
	l0.regions = cu_count(f->device); // pass-A workgroups: one per CU
	if (!plan_splits(pl, l0.regions, cu_count(f->device)) || !part_hash_fits(f->hp, l0.P))
		return pp;
	pp.tiling = part_tiling(f->hp, l0.P, base.layout, base.len);
	const uint64_t budget = scratch_budget(f);
	pp.tail = part_tail(budget);
	// (a caller-imposed budget below 2 GiB keeps its scratch for the entries: pass A then runs its plain schedule)
	pl.late_cap = budget >= (2ull << 30) ? part_late_cap() : 0;
	const uint64_t late_bytes = (uint64_t)l0.regions * 2 * pl.late_cap * sizeof(uint32_t);
	const uint64_t extra_bytes = ((pp.tail.bytes + 255) / 256) * 256 + late_bytes;
	// a shard fed every rank's reads (ShardedBloomFilter's gather mode) keeps only its window's share
	const double ppt = probes_per_tile(f, pp.tiling) * ((double)f->mod.shard_len / (double)f->mod.size);
	auto batch_bytes = [&](uint64_t t) {
		plan_caps(pl, (double)tiles_for_caps(t, l0.regions) * ppt, 0);
		pl.bytes_total += extra_bytes;
		return pl.bytes_total;
	};
	const uint64_t tiles = batch_tiles_for_budget(pp.tiling.n_tiles, budget, batch_bytes);
	if (tiles == 0)
		return pp;
	batch_bytes(tiles);
	// A call that does not fit one batch: carried batches and ONE pass C where a one-split plan allows it (part_plan.hpp);
	// counting filters included -- their carried entries keep 32 bits and exact counts, and are read once.
	// Plans with groups only: those are the filters whose sweep costs something (16 level-0 bins and more), and a call
	// then still has more pass-C launches than pass-A launches.
	const uint32_t forced = carry_enabled() ? carry_forced() : 0;
	if ((tiles < pp.tiling.n_tiles || forced) && pl.n_levels == 2 && pl.group_bins && carry_enabled()) {
		CarryGeom g;
		g.n_tiles = pp.tiling.n_tiles;
		g.probes_per_tile = ppt;
		g.regions0 = l0.regions;
		g.bins0 = l0.bins;
		g.bins1 = pl.lv[1].bins;
		g.useful1 = std::min<uint64_t>(pl.n_seg, pl.lv[1].bins);
		g.group_bins1 = pl.lv[1].alloc_bins;
		g.regions_group = pl.lv[1].regions;
		g.regions_carry = split_slices(l0.bins, l0.regions, cu_count(f->device));
		g.epc1 = part_epc(pl.lv[1].packed);
		g.extra_bytes = extra_bytes;
		const CarryPlan cp = forced ? plan_forced(g, budget, forced) : plan_call(g, budget);
		if (cp.K) {
			auto take = [](PartLevel& l, const LevelBytes& b) {
				l.cap = b.cap;
				l.cnt_bytes = b.cnt_bytes;
				l.ent_bytes = b.ent_bytes;
			};
			take(l0, cp.l0);
			take(pl.lv[1], cp.group);
			pl.carry = pl.lv[1];
			pl.carry.regions = g.regions_carry;
			pl.carry.alloc_bins = pl.carry.bins;
			pl.carry.cap = cp.block.cap;
			pl.carry.cnt_bytes = cp.carry_cnt_bytes;
			pl.carry.ent_bytes = cp.K * cp.block.ent_bytes;
			pl.carry_k = cp.K;
			pl.carry_tiles = cp.tiles_carried;
			pl.bytes_total = cp.bytes_total;
		}
	}
	// AUTO: a batch that the scratch budget has cut small is not worth a sweep of the array either (the rule
	// want_partitioned applies to the whole call, applied to one batch): a filter that nearly fills the HBM
	// leaves a few GB for scratch, and the direct kernels are then the faster path
	// (a carried plan sweeps once for the whole call, which want_partitioned has weighed already)
	if (mode == BTLBF_INSERT_AUTO && !pl.carry_k && tiles < pp.tiling.n_tiles &&
	    (double)tiles * ppt < auto_ratio * (double)f->local_bytes)
		return pp;
	pl.tiles_per_batch = pl.carry_k ? pp.tiling.n_tiles : tiles;
	if (!f->part.grow(pl.bytes_total, f->device))
		return pp; // no room for scratch: the caller falls back to the direct kernels
	if (getenv("BTLBF_PLAN_LOG")) // diagnostic: the plan of every call, one line on stderr
		fprintf(stderr,
		        "btlbf plan: budget %llu tiles %llu carried batches %u of %llu tiles (independent batches of %llu) scratch %llu "
		        "level0 %llu group %llu carried %llu caps %u %u %u\n",
		        (unsigned long long)budget, (unsigned long long)pp.tiling.n_tiles, pl.carry_k, (unsigned long long)pl.carry_tiles,
		        (unsigned long long)pl.tiles_per_batch, (unsigned long long)pl.bytes_total,
		        (unsigned long long)(l0.cnt_bytes + l0.ent_bytes),
		        (unsigned long long)(pl.n_levels >= 2 ? pl.lv[1].cnt_bytes + pl.lv[1].ent_bytes : 0),
		        (unsigned long long)(pl.carry_k ? pl.carry.cnt_bytes + pl.carry.ent_bytes : 0), l0.cap,
		        pl.n_levels >= 2 ? pl.lv[1].cap : 0, pl.carry_k ? pl.carry.cap : 0);
	pp.extra = carve_levels(pl, static_cast<uint8_t*>(f->part.p), 0);
	if (pl.carry_k) {
		pl.carry.cnt = reinterpret_cast<uint32_t*>(pp.extra);
		pl.carry.ent = reinterpret_cast<uint32_t*>(pp.extra + pl.carry.cnt_bytes);
		pp.extra += pl.carry.cnt_bytes + pl.carry.ent_bytes;
	}
	pl.late_buf = pl.late_cap ? reinterpret_cast<uint32_t*>(pp.extra + ((pp.tail.bytes + 255) / 256) * 256) : nullptr;
	pp.ok = true;
	return pp;
}

// ---- multi-GPU routing (SURVEY.md 8e on the partitioned pipeline) -------------------------------------
// The GLOBAL filter (size = f->mod.size, a power of two) is cut into B = 512 (or 1024) level-0 bins; with W shards
// owner g holds bins [g*1024/W, (g+1)*1024/W).  An origin partitions its probes into those bins (pass
// A, regions = its CU count); the block of one owner is contiguous, so the exchange is a fixed-size
// all-to-all of [B/W bins][regions][cap][kChunk] uint32 plus the entry counts.
struct RoutePlan {
	uint32_t n_windows = 1;        // position windows routed one after the other (see route_plan)
	uint32_t shards_per_window = 1;
	uint32_t window_shift = 0;     // log2(positions per window)
	uint32_t bins = 1024; // level-0 bins over ONE window of the global position space
	uint32_t shift0 = 0;  // log2(positions per level-0 bin)
	uint32_t bins_per_shard = 0;
	uint32_t regions = 0;
	uint32_t cap = 0;
	uint64_t ent_bytes_per_shard = 0, cnt_bytes_per_shard = 0;
	PartPlan owner; // the owner's levels below the level-0 bins of its shard (plan_routed with want_owner)
};

// An entry is the offset of a position inside its level-0 bin and has 32 bits; pass A stages at most 1024
// bins.  So one routing pass covers at most 2^42 positions: a larger filter (C4: 2^43 bits on 8 GPUs) is
// routed in WINDOWS of 2^42 positions, one pass A per window over the same reads (its WINDOW variant keeps
// the probes inside the window; the hashing is repeated, the partitioning is not).  A window is owned by
// n_shards / n_windows consecutive shards, and only they receive blocks of that window's pass.
int route_plan(const btlbf_filter* f, uint64_t len, const LayoutParams& lay, unsigned n_shards, RoutePlan& rp)
{
	const uint64_t M = f->mod.size;
	if (!f->mod.pow2 || n_shards == 0 || (n_shards & (n_shards - 1)) || n_shards > 1024)
		return fail(BTLBF_EINVAL, "routing needs a filter whose global size and shard count are powers of two");
	if (!part_supported(f->hp) || !part_hash_fits(f->hp, 1024))
		return fail(BTLBF_EINVAL, "routing does not support this hash configuration");
	const unsigned lm = ceil_log2(M);
	unsigned max_window = 42; // BTLBF_ROUTE_WINDOW_BITS exists for tests: small filters then exercise several windows
	if (const char* e = getenv("BTLBF_ROUTE_WINDOW_BITS")) {
		const int v = atoi(e);
		if (v >= 20 && v <= 42)
			max_window = (unsigned)v;
	}
	rp.window_shift = std::min(lm, max_window);
	rp.n_windows = 1u << (lm - rp.window_shift);
	if (rp.n_windows > n_shards)
		return fail(BTLBF_EINVAL, "routing a 2^%u-bit filter needs at least %u shards (windows of 2^%u positions)", lm,
		            rp.n_windows, rp.window_shift);
	rp.shards_per_window = n_shards / rp.n_windows;
	// 512 level-0 bins per window (64-entry LDS rings at the origin: few late entries) as long as an entry
	// fits 32 bits, else 1024.  BTLBF_ROUTE_BINS (power of two) exists for tests: fewer bins make small
	// filters exercise the two-split and 32-bit-entry geometries of a 1 TiB filter on 8 GPUs
	rp.bins = rp.window_shift - 9 <= 32 && rp.shards_per_window <= 512 ? 512 : 1024;
	if (const char* e = getenv("BTLBF_ROUTE_BINS")) {
		const unsigned b = (unsigned)atoi(e);
		if (b >= rp.shards_per_window && b <= 1024 && !(b & (b - 1)))
			rp.bins = b;
	}
	const unsigned lw = rp.window_shift, lb = ceil_log2(rp.bins);
	const unsigned seg_min = f->kind == BTLBF_COUNTING8 ? 16 : 19; // positions in a 64 KiB segment
	if (lw < lb + seg_min || lw - lb > 32 || rp.bins < rp.shards_per_window)
		return fail(BTLBF_EINVAL, "routing supports global filters of at least 2^29 bits (2^26 counters)");
	rp.shift0 = lw - lb;
	rp.bins_per_shard = rp.bins / rp.shards_per_window;
	rp.regions = cu_count(f->device);
	const PartTiling tl = part_tiling(f->hp, rp.bins, lay, len);
	const double entries = (double)tiles_for_caps(tl.n_tiles, rp.regions) * probes_per_tile(f, tl) / rp.n_windows;
	rp.cap = chunks_for(entries / ((double)rp.bins * rp.regions), 1, kChunk);
	rp.ent_bytes_per_shard = (uint64_t)rp.bins_per_shard * rp.regions * rp.cap * (kChunk * 4);
	rp.cnt_bytes_per_shard = (uint64_t)rp.bins_per_shard * rp.regions * 4;
	return BTLBF_OK;
}

// the owner's plan for blocks routed with `rp`: split levels below the level-0 bins of this shard
int owner_plan(btlbf_filter* f, const RoutePlan& rp, const LayoutParams& lay, uint64_t plan_len, unsigned n_blocks,
               unsigned n_shards, PartPlan& pl)
{
	if (!plan_segments(f->mod.shard_len, pl, f->kind == BTLBF_COUNTING8 ? 0 : 3))
		return fail(BTLBF_EINVAL, "shard too large for the partitioned pipeline");
	pl.lv[0].bins = rp.bins_per_shard;
	pl.lv[0].shift = rp.shift0;
	pl.lv[0].regions = rp.regions * n_blocks;
	if (pl.lv[0].shift < pl.seg_shift || !plan_splits(pl, pl.lv[0].regions, cu_count(f->device)))
		return fail(BTLBF_EINVAL, "unsupported shard geometry");
	// every origin sends about entries/n_shards to this shard; n_blocks origins
	const PartTiling tl = part_tiling(f->hp, rp.bins, lay, plan_len);
	const double entries = (double)tiles_for_caps(tl.n_tiles, rp.regions) * probes_per_tile(f, tl) * n_blocks / n_shards;
	plan_caps(pl, entries, 1);
	return BTLBF_OK;
}

LayoutParams layout_params(const btlbf_layout* layout)
{
	LayoutParams lay{nullptr, 0, 0};
	if (layout) {
		lay.n_seqs = layout->n_seqs;
		lay.read_len = layout->starts ? 0 : layout->read_len;
		lay.starts = layout->starts;
	}
	return lay;
}

// the plan of a routed pass, made once per call: the exchange geometry and, for `want_owner`, the owner's levels below
// it for blocks of n_blocks origins (0: of every shard)
int plan_routed(btlbf_filter* f, uint64_t plan_len, const LayoutParams& lay, unsigned n_shards, unsigned n_blocks,
                bool want_owner, RoutePlan& rp)
{
	if (!f)
		return fail(BTLBF_EINVAL, "null argument");
	int rc = route_plan(f, plan_len, lay, n_shards, rp);
	if (rc || !want_owner)
		return rc;
	return owner_plan(f, rp, lay, plan_len, n_blocks ? n_blocks : n_shards, n_shards, rp.owner);
}

// the owner's passes over level-0 bins [first_bin, first_bin + n_bins) of blocks routed with `rp`
int apply_routed(btlbf_filter* f, RoutePlan& rp, const void* recv_ent, const void* recv_cnt, unsigned n_blocks,
                 unsigned first_bin, unsigned n_bins, unsigned n_shards, int query, uint64_t* fail_list, uint64_t fail_cap,
                 uint64_t* fail_count, void* stream)
{
	PartPlan& pl = rp.owner;
	if (!recv_ent || !recv_cnt || n_blocks == 0)
		return fail(BTLBF_EINVAL, "null argument");
	if (f->shard_count != n_shards)
		return fail(BTLBF_EINVAL, "filter is shard %u of %u, not of %u", f->shard_index, f->shard_count, n_shards);
	if (query && (!fail_list || !fail_count))
		return fail(BTLBF_EINVAL, "query needs a fail list");
	const uint32_t group = pl.group(rp.bins_per_shard);
	if (n_bins == 0 || first_bin + n_bins > rp.bins_per_shard || first_bin % group || (n_bins % group && first_bin + n_bins != rp.bins_per_shard))
		return fail(BTLBF_EINVAL, "bins [%u, +%u) are not whole groups of %u of this shard's %u level-0 bins", first_bin,
		            n_bins, group, rp.bins_per_shard);
	DeviceGuard g(f->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	MATERIALIZE(f, s);
	if (!f->part.grow(pl.bytes_total, f->device))
		return fail(BTLBF_ENOMEM, "no room for %llu bytes of partition scratch", (unsigned long long)pl.bytes_total);
	carve_levels(pl, static_cast<uint8_t*>(f->part.p), 1);
	PartSide sd = part_side(f); // incrementAll / counter >= threshold at the owner
	sd.fail_list = fail_list;
	sd.fail_count = reinterpret_cast<unsigned long long*>(fail_count);
	sd.fail_cap = fail_cap;
	PartIn in0{n_blocks, n_bins, rp.regions, rp.cap, static_cast<const uint32_t*>(recv_cnt),
	           static_cast<const uint32_t*>(recv_ent)};
	return run_levels(f, pl, in0, sd, query, s, first_bin, n_bins);
}

} // namespace

namespace btlbf {

// decide between the direct (atomicOr per probe) and the partitioned insert
// bit filters: insert; counting filters: incrementAll only (the conservative update of `insert` needs
// the minimum over a k-mer's h counters, which live in different segments)
bool want_partitioned(const btlbf_filter* f, uint64_t len, int counting_op)
{
	if (f->insert_mode == BTLBF_INSERT_DIRECT)
		return false;
	if (f->kind == BTLBF_COUNTING8 ? counting_op != BTLBF_INCREMENT_ALL : f->kind != BTLBF_BLOOM)
		return false;
	if (!part_supported(f->hp) || len == 0)
		return false;
	if (f->insert_mode == BTLBF_INSERT_PARTITIONED)
		return true;
	// auto: one sweep of the local array (read + write) must be cheaper than the random atomics it
	// replaces: ~ 2*bytes/5.8e12 s against probes/21e9 s (kAutoInsertRatio); and the batch must be big
	// enough to be worth five launches
	return worth_sweep(f, local_probes(f, len), kAutoInsertRatio);
}

int partitioned_insert(btlbf_filter* f, const SeqArgs& base, hipStream_t s, bool* done)
{
	*done = false;
	// A pending btlbf_clear is carried out by the first batch itself: pass C builds every segment from zero in
	// LDS and writes it -- no memset of the array and no read sweep for that batch.  Pass C would also wipe what
	// the overflow paths of passes A and B write straight into the array, so a fresh batch reports those entries
	// as explicit positions instead (as the multi-GPU routing does) and they are applied after its last pass C;
	// more of them than the list holds (heavily skewed input) and the batch is redone the ordinary way.
	PartPrep pp = part_prepare(f, base, f->insert_mode, kAutoInsertRatio);
	if (!pp.ok)
		return BTLBF_OK;
	PartPlan& pl = pp.pl;
	const uint64_t total_tiles = pp.tiling.n_tiles;
	// unit by unit (part_unit): under a carried plan the fresh state, the spill list and the retry belong to the call
	for (uint64_t t0 = 0; t0 < total_tiles; t0 += pl.tiles_per_batch) {
		const PartUnit u = part_unit(pl, total_tiles, t0);
		for (int attempt = 0; attempt < 2; ++attempt) {
			const bool fresh = f->lazy_zero;
			PartSide sd = part_side(f, &pl);
			if (fresh) {
				HIP_TRY(order_after_clear(f, s)); // this batch IS the clear: after the point it was asked for
				sd.fresh = 1;
				sd.spill_count = reinterpret_cast<unsigned long long*>(pp.extra);
				sd.spill_list = reinterpret_cast<uint64_t*>(pp.extra + 256);
				sd.spill_cap = pp.tail.spill_cap;
				HIP_TRY(hipMemsetAsync(sd.spill_count, 0, 8, s));
			}
			if (int rc = run_unit(f, pl, base, u, sd, 0, s))
				return rc;
			if (!fresh)
				break;
			f->lazy_zero = false; // every segment has been written
			unsigned long long n_spill = 0;
			hipError_t e = hipMemcpyAsync(&n_spill, sd.spill_count, 8, hipMemcpyDeviceToHost, s);
			if (e == hipSuccess)
				e = hipStreamSynchronize(s);
			if (e == hipSuccess && n_spill <= pp.tail.spill_cap) {
				e = launch_spill(f->d_data, sd.spill_list, n_spill, f->mod.shard_lo, f->mod.shard_len, 0, part_side(f), s);
				if (e == hipSuccess)
					break;
			}
			if (e != hipSuccess) { // the batch is half applied: back to a defined (empty) state
				f->lazy_zero = true;
				return fail(BTLBF_EHIP, "fresh partitioned insert: %s", hipGetErrorString(e));
			}
			HIP_TRY(hipMemsetAsync(f->d_data, 0, f->alloc_bytes, s)); // start over, the ordinary way
		}
	}
	*done = true;
	return BTLBF_OK;
}

// Partitioned contains(): positions are partitioned exactly as for insert and
// TESTED against each segment in LDS; positions found clear go to a (small) fail list.  A batch
// without failures is finished: every clean window hits.  Otherwise the failed positions become a
// cache-resident hash set and one more hashing pass clears the windows that own one of them.  Too
// many failures (a miss-heavy batch) and the batch is redone by the direct gather kernel.
// hit_bits (device) is required; valid_bits and counts are optional.
// base.read_mask, defer_hit_count and level0 (see part_prepare) serve the SplitCold route alone and are described at its
// call (host_query.cpp).
int part_query(btlbf_filter* f, const SeqArgs& base, uint8_t* hit_bits, uint8_t* valid_bits, uint64_t* counts,
               hipStream_t s, bool* done, bool defer_hit_count, const PartPlan* level0)
{
	*done = false;
	PartPrep pp = part_prepare(f, base, f->query_mode, kAutoQueryRatio, level0);
	if (!pp.ok)
		return BTLBF_OK;
	PartPlan& pl = pp.pl;
	const uint64_t total_tiles = pp.tiling.n_tiles;
	PartSide sd = part_side(f, &pl); // (pos_base: the fail set is keyed by global position)
	sd.fail_count = reinterpret_cast<unsigned long long*>(pp.extra);
	sd.fail_list = reinterpret_cast<uint64_t*>(pp.extra + 256);
	sd.fail_cap = pp.tail.fail_cap;
	const int direct_op = direct_query_op(f);
	uint64_t* table = sd.fail_list + pp.tail.fail_cap;
	uint64_t* ctl = reinterpret_cast<uint64_t*>(pp.extra + 64); // two words of stream-side control next to the fail count
	if (counts)
		HIP_TRY(hipMemsetAsync(counts, 0, 16, s));
	const uint64_t seq_tw = (uint64_t)seq_tile_windows();
	const uint64_t seq_tiles_all = (base.len + seq_tw - 1) / seq_tw;
	// unit by unit (part_unit): under a carried plan the fail list is the call's, and one resolve step follows its
	// single test pass
	for (uint64_t t0 = 0; t0 < total_tiles; t0 += pl.tiles_per_batch) {
		const PartUnit u = part_unit(pl, total_tiles, t0);
		SeqArgs a = base;
		a.hit_bits = hit_bits;
		a.valid_bits = valid_bits;
		a.counts = counts; // pass A adds the clean-window count to counts[0]
		HIP_TRY(hipMemsetAsync(sd.fail_count, 0, 8, s));
		if (int rc = run_unit(f, pl, a, u, sd, 1, s))
			return rc;
		// redo / refine this unit's window range with the direct kernels: their tiles that overlap the
		// unit's bytes.  A tile more at either end is harmless: a failed position is a bit that IS clear,
		// so clearing any window that owns it is right, and a direct redo computes the true answer.
		// What happens is decided on the device (GATE_*): no failed position -> nothing; up to fail_cap -> they become
		// a hash set and one hashing pass clears the windows that own one; more -> the range is redone by the direct
		// kernel.  All launches are issued, the ones decided against return at once: no host round trip per batch.
		const uint64_t first = u.first * pp.tiling.tile_bytes / seq_tw;
		const uint64_t end_b = std::min<uint64_t>(base.len, (u.first + u.n) * (uint64_t)pp.tiling.tile_bytes);
		const uint64_t n = std::min<uint64_t>((end_b + seq_tw - 1) / seq_tw, seq_tiles_all) - first;
		ProfSpan ps(f, BTLBF_PROF_QUERY_RESOLVE, s);
		HIP_TRY(launch_failset_auto(sd.fail_list, sd.fail_count, pp.tail.fail_cap, table, pp.tail.table_slots, ctl, s));
		SeqArgs d = base;
		d.first_tile = first;
		d.n_tiles = n;
		d.hit_bits = hit_bits;
		d.valid_bits = nullptr;
		d.counts = nullptr;
		d.gate = ctl;
		d.gate_mode = GATE_REDO;
		REQUIRE_MATERIALIZED(f);
		HIP_TRY(launch_seq_op(direct_op, d, s));
		d.buckets = table;
		d.gate_mode = GATE_RESOLVE;
		HIP_TRY(launch_seq_op(OP_BF_RESOLVE, d, s));
	}
	if (counts && !defer_hit_count) // hits = set bits of the final bitmap
		HIP_TRY(launch_popcount(hit_bits, ((base.len + 63) / 64) * 8, 0, 0,
		                        reinterpret_cast<unsigned long long*>(counts) + 1, s));
	*done = true;
	return BTLBF_OK;
}

} // namespace btlbf

extern "C" int btlbf_route_plan(btlbf_filter* f, uint64_t len, const btlbf_layout* layout, unsigned n_shards,
                                uint64_t* ent_bytes_per_shard, uint64_t* cnt_bytes_per_shard)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_route_plan");
	if (!f || !ent_bytes_per_shard || !cnt_bytes_per_shard)
		return fail(BTLBF_EINVAL, "null argument");
	RoutePlan rp;
	if (int rc = plan_routed(f, len, layout_params(layout), n_shards, 0, false, rp))
		return rc;
	*ent_bytes_per_shard = rp.ent_bytes_per_shard;
	*cnt_bytes_per_shard = rp.cnt_bytes_per_shard;
	return BTLBF_OK;
}

// planning only (no device needed): the read grid pass A would use for fixed-length reads
extern "C" int btlbf_plan_read_grid(unsigned kmer_size, unsigned hash_num, unsigned read_len, unsigned level0_bins,
                                    uint32_t* out4)
{
	if (!out4 || kmer_size == 0 || hash_num == 0 || level0_bins == 0 || level0_bins > 1024)
		return fail(BTLBF_EINVAL, "btlbf_plan_read_grid: bad argument");
	HashParams hp;
	fill_hash_params(hp, kmer_size, hash_num);
	PartGrid g;
	(void)part_read_grid(hp, level0_bins, LayoutParams{nullptr, 0, read_len}, &g);
	out4[0] = g.reads;
	out4[1] = g.gpr;
	out4[2] = g.lpad;
	out4[3] = g.cap;
	return BTLBF_OK;
}

// planning only (no device needed): does pass A fit the LDS for plain ntHash at this k, and with what front end
extern "C" int btlbf_plan_pass_a(unsigned kmer_size, unsigned hash_num, unsigned level0_bins, uint32_t* out4)
{
	if (!out4 || kmer_size == 0 || hash_num == 0 || level0_bins == 0 || level0_bins > 1024)
		return fail(BTLBF_EINVAL, "btlbf_plan_pass_a: bad argument");
	HashParams hp;
	fill_hash_params(hp, kmer_size, hash_num);
	part_front_plan(hp, level0_bins, out4);
	return BTLBF_OK;
}

extern "C" int btlbf_route_windows(btlbf_filter* f, unsigned n_shards, unsigned* n_windows,
                                   unsigned* shards_per_window)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_route_windows");
	if (!f || !n_windows || !shards_per_window)
		return fail(BTLBF_EINVAL, "null argument");
	RoutePlan rp;
	if (int rc = plan_routed(f, 1, layout_params(nullptr), n_shards, 0, false, rp))
		return rc;
	*n_windows = rp.n_windows;
	*shards_per_window = rp.shards_per_window;
	return BTLBF_OK;
}

extern "C" int btlbf_route_seqs(btlbf_filter* f, const char* seq, uint64_t len, const btlbf_layout* layout,
                                uint64_t plan_len, unsigned n_shards, unsigned window, int query, void* send_ent,
                                void* send_cnt, uint64_t* hit_bits, uint64_t* valid_bits, uint64_t* counts,
                                uint64_t* spill_list, uint64_t spill_cap, uint64_t* spill_count, void* stream)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_route_seqs");
	int rc = seq_precheck(f);
	if (rc)
		return rc;
	if (!send_ent || !send_cnt || !spill_list || !spill_count)
		return fail(BTLBF_EINVAL, "null argument");
	DeviceGuard g(f->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	SeqView v;
	if ((rc = make_view(v, seq, len, layout, BTLBF_DEVICE, s)))
		return rc;
	RoutePlan rp;
	if ((rc = plan_routed(f, plan_len, v.lay, n_shards, 0, false, rp)))
		return rc;
	if (window >= rp.n_windows)
		return fail(BTLBF_EINVAL, "window %u of %u", window, rp.n_windows);
	SeqArgs a = base_args(f, v, len);
	// positions of the GLOBAL filter, those inside this window (all of them when there is one window)
	fill_mod(a.mod, f->mod.size, (uint64_t)window << rp.window_shift, 1ull << rp.window_shift);
	a.hit_bits = reinterpret_cast<uint8_t*>(hit_bits);
	a.valid_bits = reinterpret_cast<uint8_t*>(valid_bits);
	a.counts = counts;
	a.first_tile = 0;
	a.n_tiles = part_tiling(f->hp, rp.bins, v.lay, len).n_tiles;
	PartOut out{rp.bins, rp.regions, rp.cap, 0, static_cast<uint32_t*>(send_cnt), static_cast<uint32_t*>(send_ent)};
	PartSide sd = part_side(f); // (pass A leaves the array alone: whatever misses its rings is spilled)
	sd.spill_list = spill_list;
	sd.spill_count = reinterpret_cast<unsigned long long*>(spill_count);
	sd.spill_cap = spill_cap;
	sd.pos_base = a.mod.shard_lo; // spilled entries travel as global positions, and their bins are this window's
	// spill_count and counts ACCUMULATE over the batches of a pass (the caller zeroes them once): no
	// host round trip per batch, so the exchange of one batch can overlap the hashing of the next
	if (a.n_tiles == 0) { // nothing to hash: still publish empty regions
		HIP_TRY(hipMemsetAsync(send_cnt, 0, (size_t)rp.cnt_bytes_per_shard * rp.shards_per_window, s));
		return BTLBF_OK;
	}
	ProfSpan ps(f, query ? BTLBF_PROF_QUERY_HASH : BTLBF_PROF_INSERT_HASH, s);
	HIP_TRY(launch_part_hash(a, out, rp.shift0, sd, query, s));
	return BTLBF_OK;
}

extern "C" int btlbf_route_geometry(btlbf_filter* f, uint64_t plan_len, const btlbf_layout* layout, unsigned n_shards,
                                    unsigned n_blocks, uint32_t* out4)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_route_geometry");
	if (!f || !out4)
		return fail(BTLBF_EINVAL, "null argument");
	RoutePlan rp;
	if (int rc = plan_routed(f, plan_len, layout_params(layout), n_shards, n_blocks, true, rp))
		return rc;
	out4[0] = rp.bins_per_shard;
	out4[1] = rp.regions;
	out4[2] = rp.cap;
	out4[3] = rp.owner.group(rp.bins_per_shard);
	return BTLBF_OK;
}

extern "C" int btlbf_owner_scratch_bytes(btlbf_filter* f, uint64_t plan_len, const btlbf_layout* layout, unsigned n_shards,
                                         unsigned n_blocks, uint64_t* bytes)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_owner_scratch_bytes");
	if (!f || !bytes)
		return fail(BTLBF_EINVAL, "null argument");
	RoutePlan rp;
	if (int rc = plan_routed(f, plan_len, layout_params(layout), n_shards, n_blocks, true, rp))
		return rc;
	*bytes = rp.owner.bytes_total;
	return BTLBF_OK;
}

extern "C" int btlbf_apply_routed_bins(btlbf_filter* f, const void* recv_ent, const void* recv_cnt, unsigned n_blocks,
                                       unsigned first_bin, unsigned n_bins, uint64_t plan_len,
                                       const btlbf_layout* layout, unsigned n_shards, int query, uint64_t* fail_list,
                                       uint64_t fail_cap, uint64_t* fail_count, void* stream)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_apply_routed_bins");
	RoutePlan rp;
	if (int rc = plan_routed(f, plan_len, layout_params(layout), n_shards, n_blocks, true, rp))
		return rc;
	return apply_routed(f, rp, recv_ent, recv_cnt, n_blocks, first_bin, n_bins, n_shards, query, fail_list, fail_cap,
	                    fail_count, stream);
}

extern "C" int btlbf_apply_routed(btlbf_filter* f, const void* recv_ent, const void* recv_cnt, unsigned n_blocks,
                                  uint64_t plan_len, const btlbf_layout* layout, unsigned n_shards, int query,
                                  uint64_t* fail_list, uint64_t fail_cap, uint64_t* fail_count, void* stream)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_apply_routed");
	RoutePlan rp;
	if (int rc = plan_routed(f, plan_len, layout_params(layout), n_shards, n_blocks, true, rp))
		return rc;
	return apply_routed(f, rp, recv_ent, recv_cnt, n_blocks, 0, rp.bins_per_shard, n_shards, query, fail_list,
	                    fail_cap, fail_count, stream);
}

extern "C" int btlbf_apply_spill(btlbf_filter* f, const uint64_t* global_pos, uint64_t n, int query,
                                 uint64_t* fail_list, uint64_t fail_cap, uint64_t* fail_count, void* stream)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_apply_spill");
	if (!f || (n && !global_pos))
		return fail(BTLBF_EINVAL, "null argument");
	DeviceGuard g(f->device);
	MATERIALIZE(f, stream);
	PartSide sd = part_side(f);
	sd.fail_list = fail_list;
	sd.fail_count = reinterpret_cast<unsigned long long*>(fail_count);
	sd.fail_cap = fail_cap;
	HIP_TRY(launch_spill(f->d_data, global_pos, n, f->mod.shard_lo, f->mod.shard_len, query, sd,
	                     static_cast<hipStream_t>(stream)));
	return BTLBF_OK;
}

extern "C" int btlbf_resolve_seqs(btlbf_filter* f, const char* seq, uint64_t len, const btlbf_layout* layout,
                                  const uint64_t* fail_list, uint64_t n_fail, uint64_t* hit_bits, void* stream)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_resolve_seqs");
	int rc = seq_precheck(f);
	if (rc)
		return rc;
	if (!hit_bits || (n_fail && !fail_list))
		return fail(BTLBF_EINVAL, "null argument");
	if (n_fail == 0 || len == 0)
		return BTLBF_OK;
	if (n_fail > kFailCap)
		return fail(BTLBF_EINVAL, "more than %llu failed positions: use the direct query", (unsigned long long)kFailCap);
	DeviceGuard g(f->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	SeqView v;
	if ((rc = make_view(v, seq, len, layout, BTLBF_DEVICE, s)))
		return rc;
	if (!f->part.grow(kFailTableSlots * 8, f->device))
		return fail(BTLBF_ENOMEM, "no room for the failed-position set");
	SeqArgs a = base_args(f, v, len);
	fill_mod(a.mod, f->mod.size, 0, f->mod.size); // global positions
	a.hit_bits = reinterpret_cast<uint8_t*>(hit_bits);
	// the table is sized to the set (load <= 1/4): a few thousand failed positions make a table that stays in
	// L2, and every probe of every window is looked up in it
	uint64_t* table = static_cast<uint64_t*>(f->part.p);
	uint64_t slots = 1024;
	while (slots < 4 * n_fail && slots < kFailTableSlots)
		slots <<= 1;
	HIP_TRY(hipMemsetAsync(table, 0, slots * 8, s));
	HIP_TRY(launch_failset_build(fail_list, n_fail, table, slots - 1, s));
	a.buckets = table;
	a.bucket_cap = slots - 1;
	HIP_TRY(launch_seq_op(OP_BF_RESOLVE, a, s));
	return BTLBF_OK;
}
