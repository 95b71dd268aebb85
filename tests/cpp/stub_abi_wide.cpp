// tests/cpp/stub_abi_wide.cpp -- TEST-ONLY: the entry points CountingBloomFilter<T> (include/btlbf/) calls that
// tests/cpp/stub_abi.cpp does not have, so that every member of the shim links for T = uint16_t, uint32_t, uint64_t
// without a GPU (tests/test_wide_counter_abi_cpu.py).  They compute nothing: the program that links them only proves
// that the shim's calls match the header's declarations for every width.
#include "../../include/btlbf.h"

extern "C" {
unsigned btlbf_counter_bytes(const btlbf_filter*) { return 0; }
unsigned btlbf_threshold(const btlbf_filter*) { return 0; }
int btlbf_download(const btlbf_filter*, void*, uint64_t, uint64_t) { return BTLBF_EHIP; }
int btlbf_upload(btlbf_filter*, const void*, uint64_t, uint64_t) { return BTLBF_EHIP; }
int btlbf_min_count_hashes_wide(btlbf_filter*, const uint64_t*, uint64_t, void*, int, void*) { return BTLBF_EHIP; }
int btlbf_min_count_seqs_wide(btlbf_filter*, const char*, uint64_t, const btlbf_layout*, void*, uint64_t*, int, void*)
{
	return BTLBF_EHIP;
}
int btlbf_contains_seqs(btlbf_filter*, const char*, uint64_t, const btlbf_layout*, uint64_t*, uint64_t*, uint64_t*, int, void*)
{
	return BTLBF_EHIP;
}
int btlbf_filtered_popcount(btlbf_filter*, uint64_t*) { return BTLBF_EHIP; }
int btlbf_load(btlbf_filter**, int, const char*, unsigned, int) { return BTLBF_EHIP; }
int btlbf_create_from_header(btlbf_filter**, int, const char*, size_t, unsigned, int) { return BTLBF_EHIP; }
int btlbf_store(btlbf_filter*, const char*) { return BTLBF_EHIP; }
int btlbf_header(const btlbf_filter*, char*, size_t, size_t*) { return BTLBF_EHIP; }
}
