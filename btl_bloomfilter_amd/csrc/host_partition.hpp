// csrc/host_partition.hpp -- what the query routing (host_query.cpp) needs of the partitioned pipeline's planner and
// executor, all defined in host_partition.cpp: the plan types, the named rules a decision goes by, and part_query.
// Included by those two units only; the sequence path (host_seq.cpp) sees neither the plan types nor the planner.
#pragma once
#include "host_internal.hpp"

namespace btlbf {

// The tail of the partition scratch: a query's fail list + failed-position table, or a fresh insert's spill list.
// Inserts (fresh or not) and queries reserve the same tail, so that alternating between them never changes the
// scratch size (a re-allocation of ~100 GB costs seconds); a caller-imposed budget below 2 GiB gets short lists
// (more than a list holds and the batch is redone the plain way, which is always correct).
struct PartTail {
	uint64_t fail_cap, table_slots, spill_cap, bytes;
};
PartTail part_tail(uint64_t budget);

// one partition level: bins of 2^shift positions, written as regions of `cap` chunks
struct PartLevel {
	uint32_t bins = 0;    // bins at this level (covering the local array)
	uint32_t P = 0;       // bins per writer block (pass A: all of them; split: the fan-out)
	uint32_t regions = 0; // writers per bin
	uint32_t cap = 0;     // chunks per region
	uint32_t shift = 0;   // log2(positions per bin)
	uint32_t wseg = 0;    // level 0 only: bins of `wseg` segments each instead (plan_level0); `shift` is then unused
	uint32_t alloc_bins = 0; // bins the arrays hold at a time (== bins unless the level is processed in groups)
	uint32_t packed = 0;  // its chunks hold kPackChunk packed entries, not kChunk words (plan_caps decides)
	uint64_t cnt_bytes = 0, ent_bytes = 0;
	uint32_t* cnt = nullptr;
	uint32_t* ent = nullptr;
	PartOut out() const { return PartOut{P, regions, cap, packed, cnt, ent}; }
	PartIn in() const { return PartIn{1, alloc_bins, regions, cap, cnt, ent, packed}; }
};

struct PartPlan {
	uint32_t seg_shift = 19;
	uint64_t n_seg = 0;
	bool counting = false;   // the array holds counters: every level keeps 32-bit entries (plan_segments)
	uint32_t group_bins = 0; // level-0 bins split + applied together (one-split plans); 0 = all at once
	int n_levels = 0; // lv[0] = pass A output (or the exchanged data), lv[1..] = split outputs
	PartLevel lv[3];
	uint64_t tiles_per_batch = 0;
	uint64_t bytes_total = 0;
	// pass A's overlapped schedule keeps the entries that find their ring full in a late image per workgroup and
	// round parity (part_hash_inst.hip): [regions][2][late_cap] words behind the tail of the scratch
	uint32_t* late_buf = nullptr;
	uint32_t late_cap = 0;
	// A CARRIED plan (part_plan.hpp; carry_k != 0, one-split plans only): the call runs carry_k carried batches of
	// carry_tiles tiles and a final batch of the rest.  `carry` is lv[1] in its ungrouped form -- every bin of the array,
	// absolute segment numbers --, its arrays holding the carry_k blocks one after the other ([block][bin][region]).
	uint32_t carry_k = 0;
	uint64_t carry_tiles = 0;
	PartLevel carry;
	PartOut carry_out(uint32_t j) const
	{
		const uint64_t regs = (uint64_t)carry.bins * carry.regions;
		return PartOut{carry.P, carry.regions, carry.cap, carry.packed, carry.cnt + j * regs,
		               carry.ent + j * regs * carry.cap * kChunk};
	}
	PartIn carry_in() const { return PartIn{carry_k, carry.bins, carry.regions, carry.cap, carry.cnt, carry.ent, carry.packed}; }
	// level-0 bins that are split and applied together, of the n_bins0 a pass has (plans without groups: all of them)
	uint32_t group(uint32_t n_bins0) const { return n_levels >= 2 && group_bins ? group_bins : n_bins0; }
};

// AUTO's break-even between the direct query and a sweep of the array, in probes per byte of the local array
// (host_partition.cpp, at kAutoInsertRatio, says how both were measured)
constexpr double kAutoQueryRatio = 0.0165;

// the scratch a call may use: the caller's budget, or 80 % of the free HBM (the cached scratch counted as free)
uint64_t scratch_budget(btlbf_filter* f);
// probes a call over `len` bases sends to this filter's local array (a shard keeps its window's share)
double local_probes(const btlbf_filter* f, uint64_t len);
// are `probes` worth a sweep of the local array?  `ratio`: AUTO's break-even in probes per byte of it
bool worth_sweep(const btlbf_filter* f, double probes, double ratio);
// the direct kernel that answers contains() for this filter
int direct_query_op(const btlbf_filter* f);
// the figure plan_level0's batch-size rule goes by: local_probes, or what one batch of the caller's budget holds
double call_probes(const btlbf_filter* f, uint64_t len);
// the segment size and the level-0 bins (pass A's output) of this filter's local array; false = no partitioned path
bool plan_level0(const btlbf_filter* f, PartPlan& pl, double call_probes = 0);

// The partitioned contains() of `base` into hit_bits (required), valid_bits and counts (optional); *done = false: the
// scratch does not fit and nothing was launched.  base.read_mask, defer_hit_count and level0: see the definition.
int part_query(btlbf_filter* f, const SeqArgs& base, uint8_t* hit_bits, uint8_t* valid_bits, uint64_t* counts,
               hipStream_t s, bool* done, bool defer_hit_count, const PartPlan* level0);

} // namespace btlbf
