// csrc/screen_plan.hpp -- the host arithmetic of the read screen (host_screen.cpp), free of HIP so that a stand-alone
// test can walk it (tests/cpp/test_screen_plan.cpp): how the filters of a call are cut into the groups one launch of
// screen_kernel<NF> probes, and how many result rows a layout has.
#pragma once
#include <stdint.h>

namespace btlbf {

static constexpr unsigned kScreenMaxFilters = 16; // BTLBF_SCREEN_MAX_FILTERS
static constexpr unsigned kScreenMaxNF = 8;       // the widest instantiation of screen_kernel
static constexpr unsigned kScreenMaxGroups = (kScreenMaxFilters + kScreenMaxNF - 1) / kScreenMaxNF;

// Filters [first[g], first[g] + size[g]) form group g.  As few groups as the widest instantiation allows (every group
// stages and hashes the buffer once), of sizes that differ by at most one, the larger ones first: nine filters run as
// 5 + 4, not as 8 + 1 -- the same two passes over the reads, and neither keeps the registers of eight filters' probes.
struct ScreenGroups {
	unsigned n = 0;
	unsigned first[kScreenMaxGroups] = {0}, size[kScreenMaxGroups] = {0};
};

inline ScreenGroups screen_groups(unsigned n_filters)
{
	ScreenGroups g;
	if (n_filters == 0 || n_filters > kScreenMaxFilters)
		return g;
	g.n = (n_filters + kScreenMaxNF - 1) / kScreenMaxNF;
	unsigned at = 0;
	for (unsigned i = 0; i < g.n; ++i) {
		g.first[i] = at;
		g.size[i] = n_filters / g.n + (i < n_filters % g.n ? 1u : 0u);
		at += g.size[i];
	}
	return g;
}

// rows (sequences) of a buffer of `len` bytes: the offsets' count, whole reads of read_len bytes (what
// btlbf_count_per_seq counts), or -- no layout at all -- the buffer as one sequence
inline uint64_t screen_rows(bool has_starts, uint64_t n_seqs, uint32_t read_len, uint64_t len)
{
	if (has_starts)
		return n_seqs;
	return read_len ? len / read_len : 1;
}

// bytes of one column of the per-window bitmaps (a multiple of 16: the columns of a call lie behind one another)
inline uint64_t screen_col_bytes(uint64_t len) { return ((len + 63) / 64 * 8 + 15) & ~(uint64_t)15; }

} // namespace btlbf
