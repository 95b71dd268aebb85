// csrc/fold_plan.hpp -- the host arithmetic of btlbf_fold (host_algebra.cpp), free of HIP so that a stand-alone test can
// walk it (tests/cpp/test_fold_plan.cpp): what a fold refuses, the size of its result, and how its `factor` slices are
// cut into the groups of stage 1.
//
// A filter of src_bytes folds into one of S = src_bytes / factor bytes: slice j is source bytes [j * S, (j + 1) * S), and
// the result combines all of them.  fold_kernel gives every 16-byte vector of a result one thread, which walks the
// slices it is given.  When the result is large that is enough threads; when it is small (64 GiB folded to 64 KiB: 4096
// vectors) the slices are cut into `groups` runs of `per_group` consecutive slices, stage 1 folds run g into row g of a
// scratch of groups * out_alloc bytes, and stage 2 folds the rows (16-byte aligned and already masked: the same kernel).
#pragma once
#include <stdint.h>

namespace btlbf {

// stage 1 is given about this many threads (2048 resident per CU on 256 CUs), and never more rows than ...
static constexpr uint64_t kFoldTargetThreads = 1ull << 19;
// ... this (a launch's grid has the groups in y), nor more than about sqrt(factor): stage 2 walks `groups` rows per
// thread, so beyond that it would be the serial part
static constexpr uint64_t kFoldMaxGroups = 32768;
// THE BOUND: groups * (out_alloc / 16) <= kFoldTargetThreads whenever groups > 1, so the scratch never exceeds
// kFoldTargetThreads * 16 bytes = 8 MiB, whatever the filter
static constexpr uint64_t kFoldMaxScratch = kFoldTargetThreads * 16;

enum FoldRefusal { kFoldOk = 0, kFoldFactorZero, kFoldNotDivisible, kFoldResultNotConstructible };

struct FoldPlan {
	FoldRefusal refusal = kFoldOk;
	uint64_t out_positions = 0; // bits or counters of the result
	uint64_t out_bytes = 0;     // S
	uint64_t out_alloc = 0;     // S rounded up to 16
	uint64_t groups = 1;        // 1: one stage, no scratch
	uint64_t per_group = 0;     // slices of every group but the last, which has the rest (at least one)
	uint64_t scratch_bytes = 0; // groups * out_alloc, or 0
};

// ceil(sqrt(x)), as far as it matters: no further than kFoldMaxGroups
inline uint64_t fold_ceil_sqrt(uint64_t x)
{
	uint64_t r = 1;
	while (r < kFoldMaxGroups && r * r < x)
		++r;
	return r;
}

// elem_bytes: 0 for a bit filter (positions are bits), else the counter's width.  src_bytes is the whole body: positions / 8
// for a bit filter, positions * elem_bytes (so a multiple of elem_bytes) for a counting filter.
inline FoldPlan fold_plan(uint64_t src_bytes, uint64_t factor, unsigned elem_bytes)
{
	FoldPlan p;
	if (factor == 0) {
		p.refusal = kFoldFactorZero;
		return p;
	}
	const uint64_t positions = elem_bytes ? src_bytes / elem_bytes : src_bytes * 8;
	if (positions % factor) {
		p.refusal = kFoldNotDivisible;
		return p;
	}
	p.out_positions = positions / factor;
	// what the constructors make: bits in multiples of 8 (BloomFilter.hpp:391-394), counters in multiples of 8 bytes
	// (CountingBloomFilter.hpp:40-49)
	const bool constructible = elem_bytes ? p.out_positions * elem_bytes % 8 == 0 : p.out_positions % 8 == 0;
	if (p.out_positions == 0 || !constructible) {
		p.refusal = kFoldResultNotConstructible;
		return p;
	}
	p.out_bytes = elem_bytes ? p.out_positions * elem_bytes : p.out_positions / 8;
	p.out_alloc = (p.out_bytes + 15) / 16 * 16;
	const uint64_t n_vec = p.out_alloc / 16;
	uint64_t groups = kFoldTargetThreads / n_vec; // floor: the bound above
	const uint64_t root = fold_ceil_sqrt(factor);
	if (groups > root)
		groups = root;
	if (groups > kFoldMaxGroups)
		groups = kFoldMaxGroups;
	if (groups > factor)
		groups = factor;
	if (groups < 2) {
		p.groups = 1;
		p.per_group = factor;
		return p;
	}
	p.per_group = (factor + groups - 1) / groups;
	p.groups = (factor + p.per_group - 1) / p.per_group; // no empty group
	if (p.groups < 2) {
		p.groups = 1;
		p.per_group = factor;
		return p;
	}
	p.scratch_bytes = p.groups * p.out_alloc;
	return p;
}

} // namespace btlbf
