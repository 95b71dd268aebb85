// tests/cpp/test_algebra_shim.cpp -- the filter algebra of the drop-in headers (BloomFilter::merge / intersect / subtract /
// fold, CountingBloomFilter<T>::merge / fold / toBloomFilter) for tests/test_gpu_cpp_algebra.py, on stored filters that
// the Python side built from reads R1 and R2: every identity is checked here with btlbf_compare, and the numbers the
// Python side wants to see are printed.
// argv: a.bf b.bf both.bf both_half.bf ca.bf cb.bf cboth.bf cboth_half.bf   (c*: CountingBloomFilter<uint8_t>, incrementAll)
#define BTLBF_SHIM_THROW
#include <btlbf/BloomFilter.hpp>
#include <btlbf/CountingBloomFilter.hpp>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int g_fail = 0;
#define EXPECT(cond)                                                \
	do {                                                            \
		if (!(cond)) {                                              \
			std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
			++g_fail;                                               \
		}                                                           \
	} while (0)

static bool same(btlbf_filter* a, btlbf_filter* b)
{
	uint64_t d[3] = {1, 1, 1};
	return btlbf_compare(a, b, d) == BTLBF_OK && d[0] == 0;
}

int main(int argc, char** argv)
{
	if (argc != 9)
		return 2;
	try {
		const BloomFilter a(argv[1]), b(argv[2]), both(argv[3]), half(argv[4]);
		{
			BloomFilter u(argv[1]);
			u.merge(b);
			EXPECT(same(u.handle(), both.handle()) && u.getPop() == both.getPop());
			u.intersect(a); // (a | b) & a == a
			EXPECT(same(u.handle(), a.handle()));
			BloomFilter v(argv[3]);
			v.subtract(std::vector<const BloomFilter*>{ &b }); // ((a | b) - b) | b == a | b, and the difference is inside a
			uint64_t d[3];
			EXPECT(btlbf_compare(v.handle(), a.handle(), d) == BTLBF_OK && d[1] == 0);
			v.merge(std::vector<const BloomFilter*>{ &b, &a });
			EXPECT(same(v.handle(), both.handle()));
			std::printf("union_pop %llu\n", (unsigned long long)v.getPop());
		}
		{
			BloomFilter f = both.fold(2);
			EXPECT(f.getFilterSize() * 2 == both.getFilterSize() && f.getHashNum() == both.getHashNum() &&
			       f.getKmerSize() == both.getKmerSize());
			EXPECT(same(f.handle(), half.handle()));
			std::printf("fold_pop %llu\n", (unsigned long long)f.getPop());
		}
		const unsigned thr = 2;
		const CountingBloomFilter<uint8_t> ca(argv[5], thr), cb(argv[6], thr), cboth(argv[7], thr), chalf(argv[8], thr);
		{
			CountingBloomFilter<uint8_t> m(argv[5], thr);
			m.merge(cb);
			EXPECT(same(m.handle(), cboth.handle()));
			m.merge(std::vector<const CountingBloomFilter<uint8_t>*>{ &ca }, BTLBF_COMBINE_MIN); // min(a + b, a) == a
			EXPECT(same(m.handle(), ca.handle()));
			m.merge(cboth, BTLBF_COMBINE_MAX);
			EXPECT(same(m.handle(), cboth.handle()));
			CountingBloomFilter<uint8_t> f = cboth.fold(2);
			EXPECT(f.size() * 2 == cboth.size() && f.threshold() == thr && same(f.handle(), chalf.handle()));
			BloomFilter solid = cboth.toBloomFilter(); // the filter's own threshold
			EXPECT(solid.getFilterSize() == cboth.size() && solid.getPop() == cboth.filtered_popcount());
			BloomFilter any = cboth.toBloomFilter(1);
			EXPECT(any.getPop() == cboth.popCount() && any.getPop() > solid.getPop() && solid.getPop() > 0);
			std::printf("solid_pop %llu\n", (unsigned long long)solid.getPop());
		}
		bool refused = false;
		try {
			BloomFilter u(argv[1]);
			u.merge(half); // another size
		} catch (const std::exception& e) {
			refused = std::strstr(e.what(), "size") != nullptr;
		}
		EXPECT(refused);
	} catch (const std::exception& e) {
		std::fprintf(stderr, "exception: %s\n", e.what());
		return 1;
	}
	if (g_fail)
		return 1;
	std::printf("algebra shim ok\n");
	return 0;
}
