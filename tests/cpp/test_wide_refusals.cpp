// tests/cpp/test_wide_refusals.cpp -- TEST-ONLY: what a wide counting filter (BTLBF_COUNTING16 / 32 / 64) refuses, on
// a machine without a GPU.  A handle cannot be made there (btlbf_create needs the HBM), so this program builds the
// library's own filter object (csrc/host_internal.hpp) on the host -- no array behind it -- and calls the entry points
// that must answer BTLBF_EINVAL BEFORE ANY HIP CALL: with no array and no device, a call that got further would fail
// otherwise or crash.  Linked against libbtlbf.so by tests/test_wide_counter_abi_cpu.py.
#include "../../btl_bloomfilter_amd/csrc/host_internal.hpp"

#include <cstdio>
#include <cstring>

static int g_fail = 0;
#define REFUSED(call, word)                                                                                    \
	do {                                                                                                       \
		const int rc__ = (call);                                                                               \
		if (rc__ != BTLBF_EINVAL || !std::strstr(btlbf_last_error(), word)) {                                  \
			std::fprintf(stderr, "line %d: %s -> %d \"%s\"\n", __LINE__, #call, rc__, btlbf_last_error());      \
			++g_fail;                                                                                          \
		}                                                                                                      \
	} while (0)

#define EXPECT(cond)                                                      \
	do {                                                                  \
		if (!(cond)) {                                                    \
			std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
			++g_fail;                                                     \
		}                                                                 \
	} while (0)

int main()
{
	const int kinds[3] = {BTLBF_COUNTING16, BTLBF_COUNTING32, BTLBF_COUNTING64};
	for (int kind : kinds) {
		btlbf_filter f;
		f.kind = kind;
		f.device = 1 << 20; // no such device: a call that reached the device guard would say so
		f.h = 3;
		f.k = 25;
		f.size = 1024;
		f.size_bytes = f.local_bytes = 1024 * btlbf::counter_bytes(&f);
		const char* direct = "direct path only";
		EXPECT(btlbf_counter_bytes(&f) == (kind == BTLBF_COUNTING16 ? 2u : kind == BTLBF_COUNTING32 ? 4u : 8u));
		// modes: AUTO and DIRECT are accepted (AUTO means direct), an explicit PARTITIONED is not
		EXPECT(!btlbf_set_insert_mode(&f, BTLBF_INSERT_AUTO, 0) && !btlbf_set_insert_mode(&f, BTLBF_INSERT_DIRECT, 0) &&
		       !btlbf_set_query_mode(&f, BTLBF_INSERT_AUTO) && !btlbf_set_query_mode(&f, BTLBF_INSERT_DIRECT));
		REFUSED(btlbf_set_insert_mode(&f, BTLBF_INSERT_PARTITIONED, 0), direct);
		REFUSED(btlbf_set_query_mode(&f, BTLBF_INSERT_PARTITIONED), direct);
		EXPECT(f.insert_mode == BTLBF_INSERT_DIRECT && f.query_mode == BTLBF_INSERT_DIRECT);
		// the byte forms of the minimum counts: nothing written
		uint8_t out[64];
		std::memset(out, 0xA5, sizeof out);
		uint64_t rows[6] = {1, 2, 3, 4, 5, 6};
		REFUSED(btlbf_min_count_seqs(&f, "ACGTACGTACGTACGTACGTACGTACGTACGT", 32, nullptr, out, nullptr, BTLBF_HOST, nullptr), "_wide");
		REFUSED(btlbf_min_count_hashes(&f, rows, 2, out, BTLBF_HOST, nullptr), "_wide");
		for (uint8_t b : out)
			EXPECT(b == 0xA5);
		// shards, positions, routing, the micro-benchmark
		uint64_t u64 = 0;
		unsigned u1 = 0, u2 = 0;
		uint32_t out4[4];
		double sec = 0;
		REFUSED(btlbf_store_shard(&f, "/nonexistent/x.bf"), direct);
		REFUSED(btlbf_positions_seqs(&f, "ACGT", 4, nullptr, 1, &u64, nullptr, 1, &u64, nullptr, nullptr), direct);
		REFUSED(btlbf_insert_positions(&f, rows, 1, nullptr), direct);
		REFUSED(btlbf_test_positions(&f, rows, 1, out, nullptr), direct);
		REFUSED(btlbf_route_plan(&f, 1000, nullptr, 1, &u64, &u64), direct);
		REFUSED(btlbf_route_windows(&f, 1, &u1, &u2), direct);
		REFUSED(btlbf_route_seqs(&f, "ACGT", 4, nullptr, 4, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
		                         nullptr, nullptr), direct);
		REFUSED(btlbf_route_geometry(&f, 1000, nullptr, 1, 0, out4), direct);
		REFUSED(btlbf_owner_scratch_bytes(&f, 1000, nullptr, 1, 0, &u64), direct);
		REFUSED(btlbf_apply_routed_bins(&f, nullptr, nullptr, 1, 0, 1, 1000, nullptr, 1, 0, nullptr, 0, nullptr, nullptr), direct);
		REFUSED(btlbf_apply_routed(&f, nullptr, nullptr, 1, 1000, nullptr, 1, 0, nullptr, 0, nullptr, nullptr), direct);
		REFUSED(btlbf_apply_spill(&f, rows, 1, 0, nullptr, 0, nullptr, nullptr), direct);
		REFUSED(btlbf_resolve_seqs(&f, "ACGT", 4, nullptr, rows, 1, &u64, nullptr), direct);
		REFUSED(btlbf_microbench(&f, 0, 1000, &u64, &sec), direct);
		btlbf_rank* r = nullptr;
		REFUSED(btlbf_rank_create(&r, &f), "bit filter");
	}
	if (g_fail) {
		std::printf("%d refusals missing\n", g_fail);
		return 1;
	}
	std::printf("all wide refusals in place\n");
	return 0;
}
