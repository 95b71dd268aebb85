// The host arithmetic of the filter algebra against brute force, stand-alone (no HIP, no library): csrc/fold_plan.hpp --
// what a fold refuses, the size of its result, groups that cover every slice exactly once, the stated bound on the
// scratch, more than one group for a small result at a large factor and one for a large result -- and csrc/algebra_swar.hpp,
// the packed-counter arithmetic and the unaligned 16-byte read the kernels are made of: every pair of byte values, the
// edges of the wider counters with their neighbours, every shift and every tail length.  Built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_fold_plan_cpu.py.
#include "../../btl_bloomfilter_amd/csrc/algebra_swar.hpp"
#include "../../btl_bloomfilter_amd/csrc/fold_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace btlbf;

static int g_fail = 0;
#define EXPECT(cond)                                                \
	do {                                                            \
		if (!(cond)) {                                              \
			if (++g_fail < 20)                                      \
				std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
		}                                                           \
	} while (0)

static uint64_t rnd_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
	uint64_t z = (rnd_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

// ---- the plan ---------------------------------------------------------------------------------------------------------
static void check_plan(uint64_t src_bytes, uint64_t factor, unsigned elem)
{
	if (elem && src_bytes % elem)
		return; // not a body of whole counters
	const FoldPlan p = fold_plan(src_bytes, factor, elem);
	const uint64_t positions = elem ? src_bytes / elem : src_bytes * 8;
	// the refusals, restated
	FoldRefusal want = kFoldOk;
	if (factor == 0)
		want = kFoldFactorZero;
	else if (positions % factor)
		want = kFoldNotDivisible;
	else if (positions / factor == 0 || (elem ? (positions / factor) * elem % 8 != 0 : (positions / factor) % 8 != 0))
		want = kFoldResultNotConstructible;
	EXPECT(p.refusal == want);
	if (p.refusal != kFoldOk)
		return;
	EXPECT(p.out_positions == positions / factor);
	EXPECT(p.out_bytes * factor == src_bytes);
	EXPECT(p.out_alloc % 16 == 0 && p.out_alloc >= p.out_bytes && p.out_alloc < p.out_bytes + 16);
	// the groups cover [0, factor) exactly once, in order, none empty
	EXPECT(p.groups >= 1 && p.groups <= kFoldMaxGroups && p.per_group >= 1);
	uint64_t covered = 0;
	for (uint64_t g = 0; g < p.groups; ++g) {
		const uint64_t j0 = g * p.per_group, j1 = std::min(j0 + p.per_group, factor);
		EXPECT(j0 == covered && j1 > j0);
		covered = j1;
	}
	EXPECT(covered == factor);
	// the scratch: none for one stage, else the rows, within the stated bound
	if (p.groups == 1) {
		EXPECT(p.scratch_bytes == 0);
	} else {
		EXPECT(p.scratch_bytes == p.groups * p.out_alloc);
		EXPECT(p.scratch_bytes <= kFoldMaxScratch);
		EXPECT(p.groups * (p.out_alloc / 16) <= kFoldTargetThreads);
		EXPECT(p.groups * p.groups <= 4 * factor); // about sqrt(factor): stage 2 is not the serial part
	}
	// a large result is one stage; a small result at a large factor is not left to a few threads
	if (p.out_alloc / 16 > kFoldTargetThreads / 2)
		EXPECT(p.groups == 1);
	if (p.out_alloc / 16 <= 4096 && factor >= 1024)
		EXPECT(p.groups >= 32);
}

static void test_plan()
{
	const uint64_t sizes[] = {1, 7, 8, 9, 15, 16, 17, 24, 64, 4099, 4104, 65536, (1u << 20) + 8, 1ull << 26, 1ull << 33, 1ull << 36};
	const uint64_t factors[] = {0, 1, 2, 3, 5, 7, 8, 64, 1000, 4096, 65536, 1u << 20, 1ull << 30};
	for (unsigned elem : {0u, 1u, 2u, 4u, 8u})
		for (uint64_t s : sizes)
			for (uint64_t f : factors) {
				check_plan(s, f, elem);             // mostly refusals
				if (f && s <= (1ull << 36) / f * 16) // a body of f slices of s bytes
					check_plan(s * f, f, elem);
			}
	for (int i = 0; i < 20000; ++i) {
		const uint64_t s = 1 + rnd() % (1 + (rnd() % 3 ? 4096 : 1 << 24)), f = 1 + rnd() % (1 + (rnd() % 2 ? 70 : 1 << 21));
		check_plan(s * f, f, (unsigned)(rnd() % 2 ? 0 : 1u << (rnd() % 4)));
	}
	// the issue's two named cases: 64 GiB to 64 KiB, and 2^39 bits by 2
	const FoldPlan small = fold_plan(1ull << 36, 1ull << 20, 0), large = fold_plan(1ull << 36, 2, 0);
	EXPECT(small.refusal == kFoldOk && small.out_bytes == 65536 && small.groups > 1 && small.groups * 4096 >= kFoldTargetThreads / 2);
	EXPECT(large.refusal == kFoldOk && large.groups == 1 && large.scratch_bytes == 0);
}

// ---- the packed arithmetic --------------------------------------------------------------------------------------------
template <int B>
static uint64_t get(uint64_t w, int i)
{
	return B == 8 ? w : (w >> (8 * B * i)) & ((1ull << (8 * B % 64)) - 1);
}
template <int B>
static void check_word(uint64_t a, uint64_t b)
{
	using S = Swar<B>;
	const uint64_t mx = B == 8 ? ~0ull : (1ull << (8 * B % 64)) - 1;
	const uint64_t add = S::add_sat(a, b), hi = S::max(a, b), lo = S::min(a, b), ge = S::ge_mask(a, b), nz = S::nonzero_top(a);
	for (int i = 0; i < 8 / B; ++i) {
		const uint64_t x = get<B>(a, i), y = get<B>(b, i);
		const unsigned __int128 sum = (unsigned __int128)x + y;
		EXPECT(get<B>(add, i) == (sum > mx ? mx : (uint64_t)sum));
		EXPECT(get<B>(hi, i) == std::max(x, y) && get<B>(lo, i) == std::min(x, y));
		EXPECT(get<B>(ge, i) == (x >= y ? mx : 0));
		EXPECT((get<B>(nz, i) >> (8 * B - 1)) == (x != 0) && (get<B>(nz, i) & (mx >> 1)) == 0);
	}
}
template <int B>
static void test_width()
{
	const uint64_t mx = B == 8 ? ~0ull : (1ull << (8 * B % 64)) - 1;
	const uint64_t edge[] = {0, 1, 2, mx / 2, mx / 2 + 1, mx - 1, mx, 0x00000000FFFFFFFFull & mx, 0xFFFFFFFF00000000ull & mx};
	// every pair of edges in one counter, with random and with extreme neighbours
	for (uint64_t x : edge)
		for (uint64_t y : edge)
			for (int i = 0; i < 8 / B; ++i)
				for (int fill = 0; fill < 4; ++fill) {
					uint64_t a = fill == 0 ? 0 : fill == 1 ? ~0ull : rnd(), b = fill == 0 ? ~0ull : fill == 1 ? 0 : rnd();
					if (B < 8) {
						const uint64_t m = mx << (8 * B * i);
						a = (a & ~m) | (x << (8 * B * i));
						b = (b & ~m) | (y << (8 * B * i));
					} else {
						a = x;
						b = y;
					}
					check_word<B>(a, b);
				}
	for (int i = 0; i < 200000; ++i) {
		uint64_t a = rnd(), b = rnd();
		if (i % 3 == 0)
			a |= rnd() | rnd(), b |= rnd(); // many counters near their maximum
		if (i % 5 == 0)
			b &= rnd() & rnd();
		check_word<B>(a, b);
	}
}

static void test_bytes_exhaustive()
{
	// every pair of byte values, in every byte of a word, between FF 00 neighbours (the pattern FF 00 01 FF among them)
	for (unsigned x = 0; x < 256; ++x)
		for (unsigned y = 0; y < 256; ++y)
			for (int i = 0; i < 8; i += 3) {
				const uint64_t m = 0xffull << (8 * i);
				const uint64_t a = (0xFF0001FFFF0001FFull & ~m) | ((uint64_t)x << (8 * i));
				const uint64_t b = (0x01FFFF0100FF01FFull & ~m) | ((uint64_t)y << (8 * i));
				check_word<1>(a, b);
			}
}

// ---- the unaligned read -------------------------------------------------------------------------------------------------
static void test_align_and_keep()
{
	unsigned char buf[48];
	for (int i = 0; i < 48; ++i)
		buf[i] = (unsigned char)(i * 7 + 1);
	uint64_t w[4];
	std::memcpy(w, buf, 32);
	for (uint32_t sh = 0; sh < 16; ++sh) {
		uint64_t w0, w1;
		align_bytes(w[0], w[1], w[2], w[3], sh, w0, w1);
		unsigned char got[16];
		std::memcpy(got, &w0, 8);
		std::memcpy(got + 8, &w1, 8);
		EXPECT(std::memcmp(got, buf + sh, 16) == 0);
		for (uint32_t n = 0; n <= 16; ++n) {
			uint64_t k0 = w0, k1 = w1;
			keep_low_bytes(k0, k1, n);
			unsigned char kept[16], want[16] = {0};
			std::memcpy(kept, &k0, 8);
			std::memcpy(kept + 8, &k1, 8);
			std::memcpy(want, buf + sh, n);
			EXPECT(std::memcmp(kept, want, 16) == 0);
		}
	}
}

int main()
{
	test_plan();
	test_width<1>();
	test_width<2>();
	test_width<4>();
	test_width<8>();
	test_bytes_exhaustive();
	test_align_and_keep();
	if (g_fail) {
		std::printf("%d fold plan / packed arithmetic checks failed\n", g_fail);
		return 1;
	}
	std::printf("fold plan test passed\n");
	return 0;
}
