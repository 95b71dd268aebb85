// tests/cpp/test_algebra_refusals.cpp -- TEST-ONLY: what btlbf_clone, btlbf_combine, btlbf_fold and btlbf_threshold_bits
// refuse, on a machine without a GPU.  A handle cannot be made there (btlbf_create needs the HBM), so this program builds
// the library's own filter object (csrc/host_internal.hpp) on the host -- no array behind it, device 1 << 20 -- and checks
// that every refusal is BTLBF_EINVAL BEFORE ANY HIP CALL, with *out set to NULL, pop_out untouched and the reason in the
// message: a call that got past the checks answers BTLBF_EHIP ("no GPU"), which the controls show.  Linked against
// libbtlbf.so by tests/test_algebra_abi_cpu.py.
#include "../../btl_bloomfilter_amd/csrc/host_internal.hpp"

#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

static int g_fail = 0;
#define EXPECT(cond)                                                \
	do {                                                            \
		if (!(cond)) {                                              \
			std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
			++g_fail;                                               \
		}                                                           \
	} while (0)

static const uint64_t kPoison = 0xA5A5A5A5A5A5A5A5ull;
static btlbf_filter* const kStale = reinterpret_cast<btlbf_filter*>(99);

static void init(btlbf_filter& f, int kind = BTLBF_BLOOM)
{
	const unsigned cb = kind == BTLBF_BLOOM ? 0 : 1u << (kind - BTLBF_COUNTING8);
	f.kind = kind;
	f.device = 1 << 20; // no such device: a call that reached the device says so
	f.h = f.hp.h = 3;
	f.k = f.hp.k = 25;
	f.thr = 0;
	f.size_bytes = f.local_bytes = 128;
	f.alloc_bytes = 128;
	f.size = cb ? 128 / cb : 1024;
	f.shard_index = 0;
	f.shard_count = 1;
	f.mod.shard_lo = 0;
	f.hp.n_seeds = 0;
	f.hp.h2 = 0;
	f.seed_strs.clear();
}

// combine(dst, srcs, n, op) is refused with `word` in the message and pop untouched
static void combine_refused(int line, btlbf_filter* dst, btlbf_filter* const* srcs, unsigned n, int op, const char* word)
{
	uint64_t pop = kPoison;
	const int rc = btlbf_combine(dst, srcs, n, op, &pop);
	if (rc != BTLBF_EINVAL || !std::strstr(btlbf_last_error(), word) || pop != kPoison) {
		std::fprintf(stderr, "line %d: combine -> %d \"%s\"\n", line, rc, btlbf_last_error());
		++g_fail;
	}
}
#define COMBINE_REFUSED(dst, srcs, n, op, word) combine_refused(__LINE__, dst, srcs, n, op, word)

// a call that makes a filter is refused with `word` in the message and *out == NULL
template <class Call>
static void make_refused(int line, Call call, const char* word)
{
	btlbf_filter* out = kStale;
	const int rc = call(&out);
	if (rc != BTLBF_EINVAL || !std::strstr(btlbf_last_error(), word) || out != nullptr) {
		std::fprintf(stderr, "line %d: -> %d \"%s\" out %p\n", line, rc, btlbf_last_error(), (void*)out);
		++g_fail;
	}
}
#define MAKE_REFUSED(call, word) make_refused(__LINE__, [&](btlbf_filter** out) { return call; }, word)
// ... and one that passes the checks reaches the device
#define MAKE_CONTROL(call)                                                                             \
	do {                                                                                               \
		btlbf_filter* out__ = kStale;                                                                  \
		btlbf_filter** out = &out__;                                                                   \
		EXPECT((call) == BTLBF_EHIP && out__ == nullptr && std::strstr(btlbf_last_error(), "no GPU")); \
	} while (0)

int main()
{
	std::vector<std::unique_ptr<btlbf_filter>> own;
	btlbf_filter* fs[18];
	for (int i = 0; i < 18; ++i) {
		own.emplace_back(new btlbf_filter);
		init(*own.back());
		fs[i] = own[i].get();
	}
	btlbf_filter* dst = fs[17];

	// ---- combine ----
	for (unsigned n : {1u, 2u, 3u, 5u, 16u}) // control: nothing to refuse -> the device guard
		for (int op : {BTLBF_COMBINE_OR, BTLBF_COMBINE_AND, BTLBF_COMBINE_ANDNOT}) {
			uint64_t pop = kPoison;
			EXPECT(btlbf_combine(dst, fs, n, op, &pop) == BTLBF_EHIP && pop == kPoison);
			EXPECT(std::strstr(btlbf_last_error(), "no GPU"));
		}
	EXPECT(btlbf_combine(dst, fs, 2, BTLBF_COMBINE_OR, nullptr) == BTLBF_EHIP); // pop_out may be null
	COMBINE_REFUSED(nullptr, fs, 2, BTLBF_COMBINE_OR, "null");
	COMBINE_REFUSED(dst, nullptr, 2, BTLBF_COMBINE_OR, "null");
	{
		btlbf_filter* with_null[3] = {fs[0], nullptr, fs[2]};
		COMBINE_REFUSED(dst, with_null, 3, BTLBF_COMBINE_OR, "null handle");
		btlbf_filter* with_dst[3] = {fs[0], fs[1], dst};
		COMBINE_REFUSED(dst, with_dst, 3, BTLBF_COMBINE_AND, "among the sources");
	}
	COMBINE_REFUSED(dst, fs, 0, BTLBF_COMBINE_OR, "n_srcs");
	COMBINE_REFUSED(dst, fs, 17, BTLBF_COMBINE_OR, "n_srcs");
	// an op that does not belong to the kind
	for (int op : {-1, 6, (int)BTLBF_COMBINE_ADD, (int)BTLBF_COMBINE_MAX, (int)BTLBF_COMBINE_MIN})
		COMBINE_REFUSED(dst, fs, 2, op, "does not belong");
	for (int kind : {BTLBF_COUNTING8, BTLBF_COUNTING16, BTLBF_COUNTING32, BTLBF_COUNTING64}) {
		init(*dst, kind);
		init(*own[0], kind);
		init(*own[1], kind);
		for (int op : {BTLBF_COMBINE_OR, BTLBF_COMBINE_AND, BTLBF_COMBINE_ANDNOT})
			COMBINE_REFUSED(dst, fs, 2, op, "does not belong");
		for (int op : {BTLBF_COMBINE_ADD, BTLBF_COMBINE_MAX, BTLBF_COMBINE_MIN}) {
			uint64_t pop = kPoison;
			EXPECT(btlbf_combine(dst, fs, 2, op, &pop) == BTLBF_EHIP && pop == kPoison);
		}
		// a source of another kind: a bit filter, and a counter of another width
		COMBINE_REFUSED(dst, fs, 3, BTLBF_COMBINE_ADD, "kind");
		init(*own[1], kind == BTLBF_COUNTING8 ? BTLBF_COUNTING16 : BTLBF_COUNTING8);
		COMBINE_REFUSED(dst, fs, 2, BTLBF_COMBINE_ADD, "kind");
		init(*dst);
		init(*own[0]);
		init(*own[1]);
	}
	// a source that differs from dst: size, local bytes, shard range, device, hash count, k, seeds
	own[1]->size = 2048;
	COMBINE_REFUSED(dst, fs, 2, BTLBF_COMBINE_OR, "size");
	own[1]->size = 1024;
	own[1]->local_bytes = 64;
	COMBINE_REFUSED(dst, fs, 2, BTLBF_COMBINE_OR, "local bytes");
	own[1]->local_bytes = 128;
	own[1]->shard_count = 2;
	COMBINE_REFUSED(dst, fs, 2, BTLBF_COMBINE_OR, "shard");
	own[1]->shard_count = 1;
	own[1]->shard_index = 1;
	COMBINE_REFUSED(dst, fs, 2, BTLBF_COMBINE_OR, "shard");
	own[1]->shard_index = 0;
	own[1]->device = (1 << 20) + 1;
	COMBINE_REFUSED(dst, fs, 2, BTLBF_COMBINE_OR, "device");
	own[1]->device = 1 << 20;
	own[1]->h = own[1]->hp.h = 4;
	COMBINE_REFUSED(dst, fs, 2, BTLBF_COMBINE_OR, "hash_num");
	own[1]->h = own[1]->hp.h = 3;
	own[1]->k = own[1]->hp.k = 31;
	COMBINE_REFUSED(dst, fs, 2, BTLBF_COMBINE_OR, "kmer_size");
	own[1]->k = own[1]->hp.k = 25;
	{
		const std::vector<std::string> seeds_a = {"1111111111110111111111111", "1111111111011111111111111", "1011111111111111111111101"};
		std::vector<std::string> seeds_b = seeds_a;
		seeds_b[1] = "1111111110111111111111111";
		auto spaced = [](btlbf_filter& f, const std::vector<std::string>& s, unsigned h2) {
			f.seed_strs = s;
			f.hp.n_seeds = (uint32_t)s.size();
			f.hp.h2 = h2;
		};
		spaced(*dst, seeds_a, 1);
		COMBINE_REFUSED(dst, fs, 1, BTLBF_COMBINE_OR, "spaced seeds"); // one with, one without
		spaced(*own[0], seeds_b, 1);
		COMBINE_REFUSED(dst, fs, 1, BTLBF_COMBINE_OR, "spaced seeds"); // other strings
		spaced(*own[0], seeds_a, 2);
		COMBINE_REFUSED(dst, fs, 1, BTLBF_COMBINE_OR, "spaced seeds"); // another h2
		spaced(*own[0], seeds_a, 1);
		EXPECT(btlbf_combine(dst, fs, 1, BTLBF_COMBINE_OR, nullptr) == BTLBF_EHIP);
		spaced(*dst, {}, 0);
		spaced(*own[0], {}, 0);
	}
	// shards of the same range combine like whole filters
	for (btlbf_filter* f : {dst, fs[0], fs[1]}) {
		f->shard_count = 4;
		f->shard_index = 1;
		f->size = 4096;
		f->mod.shard_lo = 1024;
	}
	EXPECT(btlbf_combine(dst, fs, 2, BTLBF_COMBINE_OR, nullptr) == BTLBF_EHIP);
	for (btlbf_filter* f : {dst, fs[0], fs[1]})
		init(*f);

	// ---- clone ----
	MAKE_CONTROL(btlbf_clone(out, fs[0]));
	MAKE_REFUSED(btlbf_clone(out, nullptr), "null");
	EXPECT(btlbf_clone(nullptr, fs[0]) == BTLBF_EINVAL && std::strstr(btlbf_last_error(), "null"));

	// ---- fold ----
	MAKE_CONTROL(btlbf_fold(out, fs[0], 2));
	MAKE_CONTROL(btlbf_fold(out, fs[0], 1));   // a clone
	MAKE_CONTROL(btlbf_fold(out, fs[0], 128)); // 8 bits
	MAKE_REFUSED(btlbf_fold(out, nullptr, 2), "null");
	EXPECT(btlbf_fold(nullptr, fs[0], 2) == BTLBF_EINVAL);
	MAKE_REFUSED(btlbf_fold(out, fs[0], 0), "at least 1");
	MAKE_REFUSED(btlbf_fold(out, fs[0], 3), "does not divide");
	MAKE_REFUSED(btlbf_fold(out, fs[0], 2048), "does not divide");
	MAKE_REFUSED(btlbf_fold(out, fs[0], 256), "multiple of 8"); // 4 bits
	own[0]->shard_count = 2;
	MAKE_REFUSED(btlbf_fold(out, fs[0], 2), "shard");
	MAKE_REFUSED(btlbf_fold(out, fs[0], 1), "shard");
	own[0]->shard_count = 1;
	for (int kind : {BTLBF_COUNTING8, BTLBF_COUNTING16, BTLBF_COUNTING32, BTLBF_COUNTING64}) {
		init(*own[0], kind);                      // 128 bytes of counters
		MAKE_CONTROL(btlbf_fold(out, fs[0], 16)); // 8 bytes
		MAKE_REFUSED(btlbf_fold(out, fs[0], 0), "at least 1");
		MAKE_REFUSED(btlbf_fold(out, fs[0], 3), "does not divide");
		if (kind != BTLBF_COUNTING64)
			MAKE_REFUSED(btlbf_fold(out, fs[0], 32), "multiple of 8"); // 4 bytes
		else
			MAKE_REFUSED(btlbf_fold(out, fs[0], 32), "does not divide"); // 16 counters
	}

	// ---- threshold ----
	for (int kind : {BTLBF_COUNTING8, BTLBF_COUNTING16, BTLBF_COUNTING32, BTLBF_COUNTING64}) {
		init(*own[0], kind);
		MAKE_CONTROL(btlbf_threshold_bits(out, fs[0], 2));
		MAKE_REFUSED(btlbf_threshold_bits(out, fs[0], 0), "threshold is 0");
		own[0]->thr = 3;
		MAKE_CONTROL(btlbf_threshold_bits(out, fs[0], 0)); // the filter's own
		own[0]->shard_count = 2;
		MAKE_REFUSED(btlbf_threshold_bits(out, fs[0], 2), "shard");
		own[0]->shard_count = 1;
		if (kind != BTLBF_COUNTING8) { // a counter count that is no multiple of 8: 8 bytes of wide counters
			own[0]->size_bytes = own[0]->local_bytes = 8;
			own[0]->size = 8 >> (kind - BTLBF_COUNTING8);
			MAKE_REFUSED(btlbf_threshold_bits(out, fs[0], 2), "multiple of 8");
		}
	}
	init(*own[0]);
	MAKE_REFUSED(btlbf_threshold_bits(out, fs[0], 2), "not a bit filter");
	MAKE_REFUSED(btlbf_threshold_bits(out, nullptr, 2), "null");
	EXPECT(btlbf_threshold_bits(nullptr, fs[0], 2) == BTLBF_EINVAL);

	if (g_fail) {
		std::printf("%d algebra refusals missing\n", g_fail);
		return 1;
	}
	std::printf("all algebra refusals in place\n");
	return 0;
}
