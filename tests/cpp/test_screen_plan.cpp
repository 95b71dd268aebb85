// The read screen's host arithmetic (csrc/screen_plan.hpp) against a brute-force restatement: how n filters are cut into
// the groups one launch probes, the rows of a layout, and the column stride of the bitmaps.  Built with
// -fsanitize=address,undefined by tests/test_screen_abi_cpu.py; includes nothing of the library but that header.
#include "../../btl_bloomfilter_amd/csrc/screen_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace btlbf;

static unsigned long long g_case = 0;
#define CHECK(c)                                                                                          \
	do {                                                                                                  \
		if (!(c)) {                                                                                       \
			fprintf(stderr, "%s:%d: CHECK(%s) failed in case %llu\n", __FILE__, __LINE__, #c, g_case);   \
			exit(1);                                                                                      \
		}                                                                                                 \
	} while (0)

int main()
{
	static_assert(kScreenMaxFilters == 16 && kScreenMaxNF == 8 && kScreenMaxGroups == 2, "the restatement below uses these");
	// groups: every filter in exactly one group, in order; as few groups as 8 per group allow; sizes within one of each
	// other, never growing
	for (unsigned n = 0; n <= 40; ++n) {
		g_case = n;
		const ScreenGroups g = screen_groups(n);
		if (n == 0 || n > 16) {
			CHECK(g.n == 0);
			continue;
		}
		unsigned fewest = 1;
		while (fewest * 8 < n)
			++fewest;
		CHECK(g.n == fewest && g.n <= kScreenMaxGroups);
		std::vector<int> seen(n, 0);
		unsigned lo = 99, hi = 0;
		for (unsigned i = 0; i < g.n; ++i) {
			CHECK(g.size[i] >= 1 && g.size[i] <= 8);
			CHECK(g.first[i] == (i ? g.first[i - 1] + g.size[i - 1] : 0u));
			CHECK(i == 0 || g.size[i] <= g.size[i - 1]);
			for (unsigned j = 0; j < g.size[i]; ++j) {
				CHECK(g.first[i] + j < n);
				++seen[g.first[i] + j];
			}
			lo = g.size[i] < lo ? g.size[i] : lo;
			hi = g.size[i] > hi ? g.size[i] : hi;
		}
		for (unsigned j = 0; j < n; ++j)
			CHECK(seen[j] == 1);
		CHECK(hi - lo <= 1);
	}
	// the plans the GPU tests run (tests/test_gpu_screen.py: F = 1, 2, 3, 4, 5, 8, 9, 16)
	CHECK(screen_groups(9).n == 2 && screen_groups(9).size[0] == 5 && screen_groups(9).size[1] == 4);
	CHECK(screen_groups(16).n == 2 && screen_groups(16).size[0] == 8 && screen_groups(16).first[1] == 8);
	CHECK(screen_groups(8).n == 1 && screen_groups(5).n == 1 && screen_groups(5).size[0] == 5);
	// rows: by counting whole reads one by one
	for (uint64_t len = 0; len <= 300; ++len) {
		for (uint32_t L = 0; L <= 70; ++L) {
			g_case = len * 1000 + L;
			uint64_t rows = 0;
			if (L == 0)
				rows = 1;
			else
				for (uint64_t b = 0; b + L <= len; b += L)
					++rows;
			CHECK(screen_rows(false, 12345, L, len) == rows);
			CHECK(screen_rows(true, len % 7, L, len) == len % 7);
		}
	}
	// columns: hold a bit per byte in whole 64-bit words, start on 16-byte boundaries
	for (uint64_t len = 0; len <= 5000; ++len) {
		g_case = len;
		const uint64_t c = screen_col_bytes(len);
		CHECK(c % 16 == 0 && c * 8 >= len && c >= (len + 63) / 64 * 8 && c < (len + 63) / 64 * 8 + 16);
	}
	CHECK(screen_col_bytes((1ull << 40) + 1) == (1ull << 37) + 16);
	printf("screen plan test passed\n");
	return 0;
}
