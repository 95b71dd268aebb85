// tests/cpp/test_card_refusals.cpp -- TEST-ONLY: what the btlbf_card_* calls refuse, on a machine without a GPU.  A sketch
// cannot be made there (btlbf_card_create needs the HBM), so this program builds the library's own sketch object
// (csrc/host_internal.hpp) on the host -- no table behind it, device 1 << 20 -- and checks that every refusal comes
// BEFORE ANY HIP CALL, with the outputs untouched: a call that got past the checks answers BTLBF_EHIP ("no GPU"), which
// the controls show.  Linked against libbtlbf.so by tests/test_cardinality_solve_cpu.py.
#include "../../btl_bloomfilter_amd/csrc/host_internal.hpp"

#include <cstdio>
#include <cstring>
#include <memory>

static int g_fail = 0;
#define EXPECT(cond)                                                      \
	do {                                                                  \
		if (!(cond)) {                                                    \
			std::fprintf(stderr, "line %d: %s (\"%s\")\n", __LINE__, #cond, btlbf_last_error()); \
			++g_fail;                                                     \
		}                                                                 \
	} while (0)

static const char* kSeq = "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT";
static uint64_t g_t[16];
static double g_f[16];
static uint32_t g_table[64];
static uint64_t g_tot[3];
static btlbf_card_estimate g_est;

static void poison()
{
	std::memset(g_t, 0xA5, sizeof g_t);
	std::memset(g_f, 0xA5, sizeof g_f);
	std::memset(g_table, 0xA5, sizeof g_table);
	std::memset(g_tot, 0xA5, sizeof g_tot);
	std::memset(&g_est, 0xA5, sizeof g_est);
}
static bool all_a5(const void* p, size_t n)
{
	for (size_t i = 0; i < n; ++i)
		if (static_cast<const unsigned char*>(p)[i] != 0xA5)
			return false;
	return true;
}
static bool untouched()
{
	return all_a5(g_t, sizeof g_t) && all_a5(g_f, sizeof g_f) && all_a5(g_table, sizeof g_table) &&
	       all_a5(g_tot, sizeof g_tot) && all_a5(&g_est, sizeof g_est);
}
static bool said(const char* word) { return std::strstr(btlbf_last_error(), word) != nullptr; }

static void init(btlbf_card& c, unsigned k = 25, unsigned s = 11, unsigned r = 6, int device = 1 << 20)
{
	c.k = k;
	c.sample_bits = s;
	c.table_bits = r;
	c.device = device; // no such device: a call that reached the device guard says so
}

int main(int argc, char** argv)
{
	if (argc != 2) {
		std::fprintf(stderr, "usage: test_card_refusals readable.fq\n");
		return 2;
	}
	const char* path = argv[1];
	std::unique_ptr<btlbf_card> a(new btlbf_card), b(new btlbf_card);
	init(*a);
	init(*b);
	btlbf_card* c = a.get();
	btlbf_fastx_stats st;

	// controls: nothing to refuse -> every call reaches the device guard, and still writes nothing
	poison();
	EXPECT(btlbf_card_add_seqs(c, kSeq, 40, nullptr, BTLBF_HOST, nullptr) == BTLBF_EHIP && said("no GPU"));
	{
		btlbf_layout l = {nullptr, 0, 20};
		EXPECT(btlbf_card_add_seqs(c, kSeq, 40, &l, BTLBF_DEVICE, nullptr) == BTLBF_EHIP);
	}
	EXPECT(btlbf_card_add_fastx(c, path, 0, 0, &st) == BTLBF_EHIP && said("no GPU"));
	EXPECT(btlbf_card_clear(c) == BTLBF_EHIP);
	EXPECT(btlbf_card_merge(c, b.get()) == BTLBF_EHIP);
	EXPECT(btlbf_card_download(c, g_table, g_tot) == BTLBF_EHIP);
	EXPECT(btlbf_card_upload(c, g_table, g_tot) == BTLBF_EHIP);
	EXPECT(btlbf_card_histogram(c, g_t, 3) == BTLBF_EHIP && btlbf_card_histogram(c, g_t, 16) == BTLBF_EHIP);
	EXPECT(btlbf_card_estimate_now(c, 16, &g_est, g_f) == BTLBF_EHIP);
	EXPECT(untouched());
	{ // create: the shape is checked before the device is asked for
		btlbf_card* h = reinterpret_cast<btlbf_card*>(99);
		EXPECT(btlbf_card_create(&h, 25, 11, 22, 1 << 20) == BTLBF_EHIP && h == nullptr);
	}

	// null arguments
	EXPECT(btlbf_card_add_seqs(nullptr, kSeq, 40, nullptr, BTLBF_HOST, nullptr) == BTLBF_EINVAL && said("null"));
	EXPECT(btlbf_card_add_seqs(c, nullptr, 40, nullptr, BTLBF_HOST, nullptr) == BTLBF_EINVAL && said("null"));
	EXPECT(btlbf_card_add_fastx(nullptr, path, 0, 0, nullptr) == BTLBF_EINVAL);
	EXPECT(btlbf_card_add_fastx(c, nullptr, 0, 0, nullptr) == BTLBF_EINVAL);
	EXPECT(btlbf_card_clear(nullptr) == BTLBF_EINVAL);
	EXPECT(btlbf_card_merge(nullptr, c) == BTLBF_EINVAL && btlbf_card_merge(c, nullptr) == BTLBF_EINVAL);
	EXPECT(btlbf_card_download(nullptr, g_table, g_tot) == BTLBF_EINVAL);
	EXPECT(btlbf_card_download(c, nullptr, g_tot) == BTLBF_EINVAL && btlbf_card_download(c, g_table, nullptr) == BTLBF_EINVAL);
	EXPECT(btlbf_card_upload(nullptr, g_table, g_tot) == BTLBF_EINVAL);
	EXPECT(btlbf_card_upload(c, nullptr, g_tot) == BTLBF_EINVAL && btlbf_card_upload(c, g_table, nullptr) == BTLBF_EINVAL);
	EXPECT(btlbf_card_histogram(nullptr, g_t, 8) == BTLBF_EINVAL && btlbf_card_histogram(c, nullptr, 8) == BTLBF_EINVAL);
	EXPECT(btlbf_card_estimate_now(nullptr, 8, &g_est, g_f) == BTLBF_EINVAL);
	EXPECT(btlbf_card_estimate_now(c, 8, nullptr, g_f) == BTLBF_EINVAL);
	EXPECT(btlbf_card_estimate_now(c, 8, &g_est, nullptr) == BTLBF_EINVAL && said("null"));
	EXPECT(btlbf_card_create(nullptr, 25, 11, 22, 0) == BTLBF_EINVAL);
	EXPECT(untouched());

	// the shape of a sketch
	const struct {
		unsigned k, s, r;
		const char* word;
	} bad[] = {{0, 11, 22, "kmer_size"}, {32769, 11, 22, "kmer_size"}, {25, 33, 22, "sample_bits"},
	           {25, 11, 5, "table_bits"}, {25, 11, 29, "table_bits"}};
	for (const auto& x : bad) {
		btlbf_card* h = reinterpret_cast<btlbf_card*>(99);
		EXPECT(btlbf_card_create(&h, x.k, x.s, x.r, 0) == BTLBF_EINVAL && said(x.word) && h == nullptr);
	}
	// n_hist
	for (unsigned n : {0u, 1u, 2u, 8193u, ~0u}) {
		EXPECT(btlbf_card_histogram(c, g_t, n) == BTLBF_EINVAL && said("n_hist"));
		EXPECT(btlbf_card_estimate_now(c, n, &g_est, g_f) == BTLBF_EINVAL && said("n_hist"));
		EXPECT(btlbf_card_solve(g_t, n, 0, 10, &g_est, g_f) == BTLBF_EINVAL && said("n_hist"));
	}
	EXPECT(btlbf_card_solve(g_t, 8, 33, 10, &g_est, g_f) == BTLBF_EINVAL && said("sample_bits"));
	EXPECT(btlbf_card_solve(g_t, 8, 0, 5, &g_est, g_f) == BTLBF_EINVAL && said("table_bits"));
	EXPECT(btlbf_card_solve(g_t, 8, 0, 29, &g_est, g_f) == BTLBF_EINVAL && said("table_bits"));
	EXPECT(untouched());
	// mem, and a length that is no multiple of read_len; offsets that do not span the buffer
	EXPECT(btlbf_card_add_seqs(c, kSeq, 40, nullptr, 7, nullptr) == BTLBF_EINVAL && said("mem"));
	{
		btlbf_layout l = {nullptr, 0, 30};
		EXPECT(btlbf_card_add_seqs(c, kSeq, 40, &l, BTLBF_HOST, nullptr) == BTLBF_EINVAL && said("read_len"));
		EXPECT(btlbf_card_add_seqs(c, kSeq, 40, &l, BTLBF_DEVICE, nullptr) == BTLBF_EINVAL && said("read_len"));
		const uint64_t starts[3] = {0, 10, 39};
		btlbf_layout r = {starts, 2, 0};
		EXPECT(btlbf_card_add_seqs(c, kSeq, 40, &r, BTLBF_HOST, nullptr) == BTLBF_EINVAL && said("starts"));
	}
	// an unreadable path
	EXPECT(btlbf_card_add_fastx(c, "/nonexistent/reads.fq", 0, 0, &st) == BTLBF_EIO && said("/nonexistent/reads.fq"));
	// merge: the two sketches must agree in k, sample_bits, table_bits and device; a sketch is not merged into itself
	EXPECT(btlbf_card_merge(c, c) == BTLBF_EINVAL);
	init(*b, 31);
	EXPECT(btlbf_card_merge(c, b.get()) == BTLBF_EINVAL && said("kmer_size"));
	init(*b, 25, 10);
	EXPECT(btlbf_card_merge(c, b.get()) == BTLBF_EINVAL && said("sample_bits"));
	init(*b, 25, 11, 7);
	EXPECT(btlbf_card_merge(b.get(), c) == BTLBF_EINVAL && said("table_bits"));
	init(*b, 25, 11, 6, (1 << 20) + 1);
	EXPECT(btlbf_card_merge(c, b.get()) == BTLBF_EINVAL && said("device"));
	init(*b);
	EXPECT(btlbf_card_merge(c, b.get()) == BTLBF_EHIP);

	// the solver needs no GPU: it runs here
	{
		const uint64_t t[4] = {64 - 10, 6, 3, 1};
		EXPECT(btlbf_card_solve(t, 4, 0, 6, &g_est, g_f) == BTLBF_OK && g_est.distinct > 10.0 && g_est.overflow_buckets == 1);
		EXPECT(g_f[0] == 0.0 && g_f[1] == g_est.singletons && g_f[2] > 0.0 && all_a5(g_f + 3, sizeof g_f - 3 * sizeof(double)));
	}
	if (g_fail) {
		std::printf("%d cardinality refusals missing\n", g_fail);
		return 1;
	}
	std::printf("all cardinality refusals in place\n");
	return 0;
}
