// tests/cpp/test_screen_refusals.cpp -- TEST-ONLY: what btlbf_screen_seqs and btlbf_screen_fastx_open refuse, on a
// machine without a GPU.  A handle cannot be made there (btlbf_create needs the HBM), so this program builds the
// library's own filter object (csrc/host_internal.hpp) on the host -- no array behind it, device 1 << 20 -- and checks
// that every refusal is BTLBF_EINVAL BEFORE ANY HIP CALL, with the outputs untouched: a call that got past the checks
// answers BTLBF_EHIP ("no GPU"), which the control at the top shows.  Linked against libbtlbf.so by
// tests/test_screen_abi_cpu.py.
#include "../../btl_bloomfilter_amd/csrc/host_internal.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

static int g_fail = 0;
#define EXPECT(cond)                                                      \
	do {                                                                  \
		if (!(cond)) {                                                    \
			std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
			++g_fail;                                                     \
		}                                                                 \
	} while (0)

static const char* kSeq = "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT";
static uint32_t g_hits[64], g_valid[4], g_pass[4];

static void poison_outputs()
{
	std::memset(g_hits, 0xA5, sizeof g_hits);
	std::memset(g_valid, 0xA5, sizeof g_valid);
	std::memset(g_pass, 0xA5, sizeof g_pass);
}
static bool outputs_untouched()
{
	const unsigned char *a = reinterpret_cast<unsigned char*>(g_hits), *b = reinterpret_cast<unsigned char*>(g_valid),
	                    *c = reinterpret_cast<unsigned char*>(g_pass);
	for (size_t i = 0; i < sizeof g_hits; ++i)
		if (a[i] != 0xA5)
			return false;
	for (size_t i = 0; i < sizeof g_valid; ++i)
		if (b[i] != 0xA5 || c[i] != 0xA5)
			return false;
	return true;
}

// the in-memory call and the file open with the same filters and parameters: both refuse, with `word` in the message
static void refused(int line, btlbf_filter* const* fs, unsigned n, const btlbf_screen_params* p, const char* word,
                    const char* path)
{
	poison_outputs();
	const int rc = btlbf_screen_seqs(fs, n, kSeq, 40, nullptr, p, g_hits, g_valid, g_pass, BTLBF_HOST, nullptr);
	if (rc != BTLBF_EINVAL || !std::strstr(btlbf_last_error(), word) || !outputs_untouched()) {
		std::fprintf(stderr, "line %d: screen_seqs -> %d \"%s\"\n", line, rc, btlbf_last_error());
		++g_fail;
	}
	btlbf_screen_file* h = reinterpret_cast<btlbf_screen_file*>(99);
	const int ro = btlbf_screen_fastx_open(&h, fs, n, path, 0, p, 0);
	if (ro != BTLBF_EINVAL || !std::strstr(btlbf_last_error(), word) || h != nullptr) {
		std::fprintf(stderr, "line %d: screen_fastx_open -> %d \"%s\"\n", line, ro, btlbf_last_error());
		++g_fail;
	}
	uint64_t tot[16 + 16 + 4];
	std::memset(tot, 0xA5, sizeof tot);
	const int rw = btlbf_screen_fastx(fs, n, path, 0, p, 0, tot, tot + 16, tot + 32, nullptr);
	bool clean = true;
	for (size_t i = 0; i < sizeof tot; ++i)
		clean = clean && reinterpret_cast<unsigned char*>(tot)[i] == 0xA5;
	if (rw != BTLBF_EINVAL || !clean) {
		std::fprintf(stderr, "line %d: screen_fastx -> %d \"%s\"\n", line, rw, btlbf_last_error());
		++g_fail;
	}
}
#define REFUSED(fs, n, p, word) refused(__LINE__, fs, n, p, word, path)

static void init(btlbf_filter& f, int kind = BTLBF_BLOOM)
{
	f.kind = kind;
	f.device = 1 << 20; // no such device: a call that reached the device guard says so
	f.h = 3;
	f.k = 25;
	f.size = 1024;
	f.size_bytes = f.local_bytes = 128;
	f.hp.k = 25;
	f.hp.h = 3;
	f.hp.n_seeds = 0;
	f.hp.h2 = 0;
}

int main(int argc, char** argv)
{
	if (argc != 2) {
		std::fprintf(stderr, "usage: test_screen_refusals readable.fq\n");
		return 2;
	}
	const char* path = argv[1];
	std::vector<std::unique_ptr<btlbf_filter>> own;
	for (int i = 0; i < 17; ++i) {
		own.emplace_back(new btlbf_filter);
		init(*own.back());
	}
	btlbf_filter* fs[17];
	for (int i = 0; i < 17; ++i)
		fs[i] = own[i].get();
	const btlbf_screen_params ok = {0.5, 1, 0};

	// control: nothing to refuse -> the call reaches the device guard (and still writes nothing)
	poison_outputs();
	EXPECT(btlbf_screen_seqs(fs, 2, kSeq, 40, nullptr, &ok, g_hits, g_valid, g_pass, BTLBF_HOST, nullptr) == BTLBF_EHIP);
	EXPECT(std::strstr(btlbf_last_error(), "no GPU") && outputs_untouched());
	EXPECT(btlbf_screen_seqs(fs, 16, kSeq, 40, nullptr, &ok, g_hits, g_valid, nullptr, BTLBF_HOST, nullptr) == BTLBF_EHIP);

	{ // ... and so does the file open: no handle comes back, and nothing is left running
		btlbf_screen_file* h = reinterpret_cast<btlbf_screen_file*>(99);
		EXPECT(btlbf_screen_fastx_open(&h, fs, 2, path, 0, &ok, 0) == BTLBF_EHIP && h == nullptr);
		EXPECT(std::strstr(btlbf_last_error(), "no GPU"));
	}

	// null arguments (pass_bits may be null: the control above)
	REFUSED(nullptr, 2, &ok, "null");
	REFUSED(fs, 2, nullptr, "null");
	poison_outputs();
	EXPECT(btlbf_screen_seqs(fs, 2, nullptr, 40, nullptr, &ok, g_hits, g_valid, g_pass, BTLBF_HOST, nullptr) == BTLBF_EINVAL);
	EXPECT(btlbf_screen_seqs(fs, 2, kSeq, 40, nullptr, &ok, nullptr, g_valid, g_pass, BTLBF_HOST, nullptr) == BTLBF_EINVAL);
	EXPECT(btlbf_screen_seqs(fs, 2, kSeq, 40, nullptr, &ok, g_hits, nullptr, g_pass, BTLBF_HOST, nullptr) == BTLBF_EINVAL);
	EXPECT(std::strstr(btlbf_last_error(), "null") && outputs_untouched());
	{
		btlbf_filter* with_null[3] = {fs[0], nullptr, fs[2]};
		REFUSED(with_null, 3, &ok, "null handle");
	}
	// the number of filters
	REFUSED(fs, 0, &ok, "n_filters");
	REFUSED(fs, 17, &ok, "n_filters");
	// the same handle twice, anywhere in the array
	{
		btlbf_filter* twice[4] = {fs[3], fs[1], fs[2], fs[3]};
		REFUSED(twice, 4, &ok, "twice");
	}
	// min_fraction
	for (double bad : {-0.01, 1.0001, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
		const btlbf_screen_params p = {bad, 1, 0};
		REFUSED(fs, 2, &p, "min_fraction");
	}
	for (double good : {0.0, 1.0}) {
		const btlbf_screen_params p = {good, 0, 0};
		EXPECT(btlbf_screen_seqs(fs, 2, kSeq, 40, nullptr, &p, g_hits, g_valid, g_pass, BTLBF_HOST, nullptr) == BTLBF_EHIP);
	}
	// mem, and a length that is no multiple of read_len
	poison_outputs();
	EXPECT(btlbf_screen_seqs(fs, 2, kSeq, 40, nullptr, &ok, g_hits, g_valid, g_pass, 7, nullptr) == BTLBF_EINVAL);
	{
		btlbf_layout l = {nullptr, 0, 30};
		EXPECT(btlbf_screen_seqs(fs, 2, kSeq, 40, &l, &ok, g_hits, g_valid, g_pass, BTLBF_HOST, nullptr) == BTLBF_EINVAL);
		EXPECT(std::strstr(btlbf_last_error(), "read_len") && outputs_untouched());
	}
	// a filter that is not a bit filter, of every counting kind; a shard
	for (int kind : {BTLBF_COUNTING8, BTLBF_COUNTING16, BTLBF_COUNTING32, BTLBF_COUNTING64}) {
		init(*own[1], kind);
		REFUSED(fs, 3, &ok, "not a bit filter");
		init(*own[1]);
	}
	own[2]->shard_count = 2;
	REFUSED(fs, 3, &ok, "shard");
	own[2]->shard_count = 1;
	// different devices
	own[1]->device = (1 << 20) + 1;
	REFUSED(fs, 2, &ok, "device");
	own[1]->device = 1 << 20;
	// k, hash count
	own[1]->k = own[1]->hp.k = 31;
	REFUSED(fs, 2, &ok, "kmer_size");
	own[1]->k = own[1]->hp.k = 25;
	own[1]->h = own[1]->hp.h = 4;
	REFUSED(fs, 2, &ok, "hash_num");
	own[1]->h = own[1]->hp.h = 3;
	// spaced seeds: one filter with, one without; other strings; another h2
	const std::vector<std::string> seeds_a = {"1111111111110111111111111", "1111111111011111111111111", "1011111111111111111111101"};
	std::vector<std::string> seeds_b = seeds_a;
	seeds_b[1] = "1111111110111111111111111";
	auto spaced = [](btlbf_filter& f, const std::vector<std::string>& s, unsigned h2) {
		f.seed_strs = s;
		f.hp.n_seeds = (uint32_t)s.size();
		f.hp.h2 = h2;
	};
	spaced(*own[0], seeds_a, 1);
	REFUSED(fs, 2, &ok, "spaced seeds");
	spaced(*own[1], seeds_b, 1);
	REFUSED(fs, 2, &ok, "spaced seeds");
	spaced(*own[1], seeds_a, 2);
	REFUSED(fs, 2, &ok, "spaced seeds");
	spaced(*own[1], seeds_a, 1);
	EXPECT(btlbf_screen_seqs(fs, 2, kSeq, 40, nullptr, &ok, g_hits, g_valid, g_pass, BTLBF_HOST, nullptr) == BTLBF_EHIP);
	spaced(*own[0], {}, 0);
	spaced(*own[1], {}, 0);
	// the file handle's own arguments
	{
		btlbf_screen_file* h = reinterpret_cast<btlbf_screen_file*>(99);
		EXPECT(btlbf_screen_fastx_open(nullptr, fs, 2, path, 0, &ok, 0) == BTLBF_EINVAL);
		EXPECT(btlbf_screen_fastx_open(&h, fs, 2, nullptr, 0, &ok, 0) == BTLBF_EINVAL);
		EXPECT(btlbf_screen_fastx_open(&h, fs, 2, "/nonexistent/reads.fq", 0, &ok, 0) == BTLBF_EIO && h == nullptr);
		EXPECT(std::strstr(btlbf_last_error(), "/nonexistent/reads.fq"));
	}
	if (g_fail) {
		std::printf("%d screen refusals missing\n", g_fail);
		return 1;
	}
	std::printf("all screen refusals in place\n");
	return 0;
}
