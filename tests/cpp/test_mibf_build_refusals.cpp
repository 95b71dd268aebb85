// tests/cpp/test_mibf_build_refusals.cpp -- TEST-ONLY: what btlbf_mibf_build_fastx (and the window counters) refuse at
// entry, on a machine without a GPU.  Every call names a device that does not exist, so a call that passes the entry
// checks answers BTLBF_EHIP ("no GPU") on any machine -- with or without a GPU -- and one that is refused answers its own
// code first: the checks come before any HIP call.  Both handles are poisoned before each call and must come back NULL.
// Linked against libbtlbf.so by tests/test_mibf_build_abi_cpu.py, which passes a directory to write two small files in.
#include "../../include/btlbf.h"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

// the layout the ctypes mirror (btl_bloomfilter_amd/_lib.py) is held to
static_assert(sizeof(btlbf_mibf_build_params) == 88 && offsetof(btlbf_mibf_build_params, device) == 80, "build params");
static_assert(sizeof(btlbf_mibf_build_report) == 208 && offsetof(btlbf_mibf_build_report, seconds_total) == 200, "report");

static int g_fail = 0;
static const int kNoDevice = 1 << 20;

static btlbf_mibf_build_params good()
{
	btlbf_mibf_build_params p;
	std::memset(&p, 0, sizeof p);
	p.kmer_size = 31;
	p.hash_num = 3;
	p.id_bytes = 2;
	p.occupancy = 0.3;
	p.id_mode = BTLBF_MIBF_ID_PER_FILE;
	p.first_id = 1;
	p.saturation = BTLBF_MIBF_SAT_SERIAL;
	p.device = kNoDevice;
	return p;
}

static void expect(int line, const char* const* paths, unsigned n, const btlbf_mibf_build_params* p, int code,
                   const char* word, bool null_out = false)
{
	btlbf_mibf* m = reinterpret_cast<btlbf_mibf*>(0x5a5a);
	btlbf_filter* f = reinterpret_cast<btlbf_filter*>(0xa5a5);
	btlbf_mibf_build_report rep;
	const int rc = btlbf_mibf_build_fastx(null_out ? nullptr : &m, &f, paths, n, p, &rep, nullptr);
	const char* msg = btlbf_last_error();
	if (rc != code || !std::strstr(msg, word) || (!null_out && m) || f) {
		std::fprintf(stderr, "line %d: rc %d (want %d) \"%s\" (want \"%s\") handles %p %p\n", line, rc, code, msg, word,
		             (void*)m, (void*)f);
		++g_fail;
	}
}
#define EXPECT_RC(paths, n, p, code, word) expect(__LINE__, paths, n, p, code, word)

int main(int argc, char** argv)
{
	if (argc < 2)
		return 2;
	const std::string dir = argv[1], a = dir + "/a.fa", b = dir + "/b.fa", gone = dir + "/missing.fa";
	for (const std::string& path : {a, b}) {
		FILE* fp = std::fopen(path.c_str(), "w");
		if (!fp)
			return 2;
		std::fputs(">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n", fp);
		std::fclose(fp);
	}
	const char* two[2] = {a.c_str(), b.c_str()};
	const char* last_gone[2] = {a.c_str(), gone.c_str()};
	const char* with_null[2] = {a.c_str(), nullptr};
	btlbf_mibf_build_params p = good();
	// what passes the checks reaches the device question, and only then
	EXPECT_RC(two, 2, &p, BTLBF_EHIP, "no GPU");
	// null and empty arguments
	expect(__LINE__, two, 2, &p, BTLBF_EINVAL, "null", true);
	EXPECT_RC(nullptr, 2, &p, BTLBF_EINVAL, "null or empty");
	EXPECT_RC(two, 0, &p, BTLBF_EINVAL, "null or empty");
	EXPECT_RC(two, 2, nullptr, BTLBF_EINVAL, "null or empty");
	EXPECT_RC(with_null, 2, &p, BTLBF_EINVAL, "path 1 is null");
	// an unreadable path, the last one: EIO, naming it
	EXPECT_RC(last_gone, 2, &p, BTLBF_EIO, "missing.fa");
	// the id type and the ids
	for (unsigned bad : {0u, 1u, 3u, 8u}) {
		p = good();
		p.id_bytes = bad;
		EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "id_bytes");
	}
	p = good();
	p.first_id = 0;
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "first_id");
	p = good();
	p.first_id = 0x7fff; // file 1 would get 0x8000, the mask of uint16_t
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "saturation mask 32768");
	p.first_id = 0x7ffe;
	EXPECT_RC(two, 2, &p, BTLBF_EHIP, "no GPU");
	p.first_id = 0x7fff;
	p.id_mode = BTLBF_MIBF_ID_PER_RECORD; // per record the last id is known after pass 1 only
	EXPECT_RC(two, 2, &p, BTLBF_EHIP, "no GPU");
	p = good();
	p.id_bytes = 4;
	p.first_id = 0x7fffffffu;
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "saturation mask 2147483648");
	EXPECT_RC(two, 1, &p, BTLBF_EHIP, "no GPU");
	p = good();
	p.id_mode = 2;
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "id_mode");
	p = good();
	p.saturation = 3;
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "saturation must be");
	// occupancy, where it is needed
	for (double occ : {0.0, 1.0, -0.1, 1.5, (double)NAN}) {
		p = good();
		p.occupancy = occ;
		EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "occupancy");
		p.expected_entries = 1000;
		EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "occupancy");
		p.bits = 4096; // not needed
		EXPECT_RC(two, 2, &p, BTLBF_EHIP, "no GPU");
	}
	// bits, hash_num, kmer_size
	p = good();
	p.bits = 4100;
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "not a multiple of 8");
	for (unsigned h : {0u, 9u}) {
		p = good();
		p.hash_num = h;
		EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "hash values per window");
	}
	p = good();
	p.kmer_size = 0;
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "kmer_size");
	// seeds: their count against hash_num, their length against kmer_size
	const char* seeds[2] = {"1110111", "1011101"};
	p = good();
	p.kmer_size = 7;
	p.hash_num = 2;
	p.seeds = seeds;
	p.n_seeds = 2;
	EXPECT_RC(two, 2, &p, BTLBF_EHIP, "no GPU");
	p.hash_num = 3;
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "2 spaced seeds but hash_num 3");
	p.hash_num = 2;
	p.kmer_size = 8;
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "spaced seed 0 is not of length");
	p.kmer_size = 7;
	p.seeds = nullptr;
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "given together");
	p = good();
	p.fastx_flags = 1u << 8;
	EXPECT_RC(two, 2, &p, BTLBF_EINVAL, "fastx_flags");
	// parallel saturation: a batch of 1000 bytes holds 970 windows of k = 31, the lists take 80 bytes per window for
	// h <= 5 and 16 * h beyond -- both sides of the edge; the serial order has no such bound
	for (unsigned h : {3u, 8u}) {
		const unsigned long long need = 970ull * (h == 3 ? 80 : 128);
		p = good();
		p.hash_num = h;
		p.saturation = BTLBF_MIBF_SAT_PARALLEL;
		p.batch_bytes = 1000;
		p.scratch_bytes = need;
		EXPECT_RC(two, 2, &p, BTLBF_EHIP, "no GPU");
		p.scratch_bytes = need - 1;
		EXPECT_RC(two, 2, &p, BTLBF_ENOMEM, (std::to_string(need) + " bytes would do").c_str());
		p.saturation = BTLBF_MIBF_SAT_SERIAL;
		EXPECT_RC(two, 2, &p, BTLBF_EHIP, "no GPU");
	}
	// the defaults (64 MiB batches, 2 GiB of scratch): 67108834 windows need 80 bytes each
	p = good();
	p.saturation = BTLBF_MIBF_SAT_PARALLEL;
	EXPECT_RC(two, 2, &p, BTLBF_ENOMEM, "5368706720 bytes would do");
	p.scratch_bytes = 5368706720ull;
	EXPECT_RC(two, 2, &p, BTLBF_EHIP, "no GPU");
	// the window counters
	uint64_t out2[2] = {7, 7};
	btlbf_fastx_stats st;
	if (btlbf_count_windows_seqs(0, "ACGT", 4, nullptr, out2, BTLBF_HOST, kNoDevice, nullptr) != BTLBF_EINVAL ||
	    btlbf_count_windows_seqs(2, nullptr, 4, nullptr, out2, BTLBF_HOST, kNoDevice, nullptr) != BTLBF_EINVAL ||
	    btlbf_count_windows_seqs(2, "ACGT", 4, nullptr, nullptr, BTLBF_HOST, kNoDevice, nullptr) != BTLBF_EINVAL ||
	    btlbf_count_windows_seqs(2, "ACGT", 4, nullptr, out2, 2, kNoDevice, nullptr) != BTLBF_EINVAL ||
	    btlbf_count_windows_seqs(2, "ACGT", 4, nullptr, out2, BTLBF_HOST, kNoDevice, nullptr) != BTLBF_EHIP ||
	    btlbf_count_windows_fastx(gone.c_str(), 31, 0, 0, kNoDevice, &st) != BTLBF_EIO ||
	    btlbf_count_windows_fastx(a.c_str(), 0, 0, 0, kNoDevice, &st) != BTLBF_EINVAL ||
	    btlbf_count_windows_fastx(a.c_str(), 31, 0, 0, kNoDevice, nullptr) != BTLBF_EINVAL ||
	    btlbf_count_windows_fastx(a.c_str(), 31, 0, 0, kNoDevice, &st) != BTLBF_EHIP || out2[0] != 7 || out2[1] != 7) {
		std::fprintf(stderr, "the window counters' entry checks: \"%s\"\n", btlbf_last_error());
		++g_fail;
	}
	if (g_fail) {
		std::printf("%d refusals missing\n", g_fail);
		return 1;
	}
	std::printf("all miBF build refusals in place\n");
	return 0;
}
