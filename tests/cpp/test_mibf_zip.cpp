// The mates zipper (csrc/mibf_zip.hpp) against the index-wise zip, by brute force: two record streams (record i of
// side s is the number i) cut into batches at random -- batches of 0 records and of 1 record among them, and all of one
// side delivered before the other side's first batch wherever the zipper's requests allow it -- must come out as the
// pairs (i, i), in order, each once; equal totals end with END, unequal ones with UNEQUAL, and only after every pair that
// exists has been taken.  And the closed form of the interleaved buffer's offsets (mibf_zip_starts) against the offsets
// of the buffer built by appending the mates one by one.  Host only; built with -fsanitize=address,undefined by
// tests/test_mibf_zip_cpu.py.
#include "../../btl_bloomfilter_amd/csrc/mibf_zip.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

using btlbf::MibfZip;

#define CHECK(c)                                                                     \
	do {                                                                             \
		if (!(c)) {                                                                  \
			std::printf("FAILED %s (line %d, case %d)\n", #c, __LINE__, g_case);     \
			std::exit(1);                                                            \
		}                                                                            \
	} while (0)
static int g_case = 0;

// batch sizes of one side: `total` records in batches of lo..hi, with empty batches sprinkled in
static std::vector<uint64_t> cut(std::mt19937_64& rng, uint64_t total, uint64_t lo, uint64_t hi, bool empties)
{
	std::vector<uint64_t> b;
	for (uint64_t left = total; left;) {
		if (empties && rng() % 4 == 0)
			b.push_back(0);
		uint64_t n = lo + rng() % (hi - lo + 1);
		if (n > left)
			n = left;
		b.push_back(n);
		left -= n;
	}
	if (empties && rng() % 2)
		b.push_back(0);
	return b;
}

// end_marker: the side's end comes as a batch of its own with no record and last = true (the parser's way); otherwise
// the last batch carries the flag
static void run_case(std::mt19937_64& rng, uint64_t n0, uint64_t n1, uint64_t lo, uint64_t hi, bool empties, bool end_marker)
{
	const uint64_t total[2] = {n0, n1};
	std::vector<uint64_t> batches[2] = {cut(rng, n0, lo, hi, empties), cut(rng, n1, lo, hi, empties)};
	size_t next_batch[2] = {0, 0};
	uint64_t base[2] = {0, 0}, fed[2] = {0, 0}; // the stream index of the current batch's first record; records fed
	bool ended[2] = {false, false};
	MibfZip z;
	uint64_t pairs = 0;
	const uint64_t want = n0 < n1 ? n0 : n1;
	for (int guard = 0;; ++guard) {
		CHECK(guard < 1000000);
		const MibfZip::Step st = z.step();
		if (st == MibfZip::END) {
			CHECK(n0 == n1 && pairs == n0 && ended[0] && ended[1]);
			break;
		}
		if (st == MibfZip::UNEQUAL) {
			CHECK(n0 != n1 && pairs == want); // not before every pair that exists was taken
			break;
		}
		if (st == MibfZip::TAKE) {
			const uint64_t a0 = base[0] + z.pos(0), a1 = base[1] + z.pos(1);
			const uint64_t n = z.take();
			CHECK(n >= 1 && a0 == pairs && a1 == pairs); // pair i is record i of both sides, in order
			CHECK(a0 + n <= fed[0] && a1 + n <= fed[1]); // only records that were delivered
			pairs += n;
			CHECK(z.pairs == pairs);
			continue;
		}
		const int s = st == MibfZip::NEED_1;
		CHECK(!ended[s] && z.left[s] == 0); // a side is asked only when its batch is used up, never behind its end
		base[s] = fed[s];
		if (next_batch[s] < batches[s].size()) {
			const uint64_t n = batches[s][next_batch[s]++];
			const bool last = !end_marker && next_batch[s] == batches[s].size();
			z.feed(s, n, last);
			fed[s] += n;
			ended[s] = last;
		} else {
			CHECK(end_marker || batches[s].empty());
			z.feed(s, 0, true);
			ended[s] = true;
		}
		CHECK(fed[s] <= total[s]);
	}
}

// side offsets of n records of random lengths, empty records among them, from a first offset that is not 0
static std::vector<uint64_t> side_starts(std::mt19937_64& rng, uint64_t n, uint64_t first)
{
	std::vector<uint64_t> s(n + 1, first);
	for (uint64_t i = 0; i < n; ++i)
		s[i + 1] = s[i] + (rng() % 3 == 0 ? 0 : rng() % 300);
	return s;
}

// mibf_zip_starts against the interleaved buffer built mate by mate: its offsets, and which bytes lie between them
static void zip_starts_case(std::mt19937_64& rng, uint64_t n, uint64_t first1, uint64_t first2)
{
	const std::vector<uint64_t> s1 = side_starts(rng, n, first1), s2 = side_starts(rng, n, first2);
	// a side's buffer holds, at byte j of its window, (side, j): enough to tell where every byte of the result came from
	std::vector<uint64_t> concat_starts{0};
	std::vector<std::pair<int, uint64_t>> buf;
	for (uint64_t i = 0; i < n; ++i)
		for (int side = 0; side < 2; ++side) {
			const std::vector<uint64_t>& s = side ? s2 : s1;
			for (uint64_t j = s[i]; j < s[i + 1]; ++j)
				buf.push_back({side, j});
			concat_starts.push_back(buf.size());
		}
	const std::vector<uint64_t> got = btlbf::mibf_zip_starts(s1.data(), s2.data(), n);
	CHECK(got.size() == 2 * n + 1 && concat_starts.size() == 2 * n + 1);
	for (uint64_t j = 0; j <= 2 * n; ++j)
		CHECK(got[j] == first1 + first2 + concat_starts[j]);
	// sequence 2i is mate 1 of pair i, 2i + 1 its mate 2, byte for byte
	for (uint64_t j = 0; j < 2 * n; ++j) {
		const std::vector<uint64_t>& s = j & 1 ? s2 : s1;
		CHECK(got[j + 1] - got[j] == s[j / 2 + 1] - s[j / 2]);
		for (uint64_t b = got[j] - got[0]; b < got[j + 1] - got[0]; ++b)
			CHECK(buf[b].first == (int)(j & 1) && buf[b].second == s[j / 2] + (b - (got[j] - got[0])));
	}
}

int main()
{
	std::mt19937_64 rng(12345);
	for (uint64_t n : {0, 1, 2, 63, 64, 65})
		for (g_case = 100000; g_case < 100050; ++g_case) {
			const bool window = g_case % 5 != 0; // most cases: offsets that do not start at 0
			zip_starts_case(rng, n, window ? 1 + rng() % 100000 : 0, window ? 1 + rng() % 100000 : 0);
		}
	for (g_case = 0; g_case < 20000; ++g_case) {
		const uint64_t n0 = rng() % 40;
		const uint64_t n1 = g_case % 3 == 0 ? rng() % 40 : n0; // a third of the cases with (mostly) unequal totals
		const uint64_t lo = 1, hi = 1 + rng() % 12;
		run_case(rng, n0, n1, lo, hi, g_case % 2 == 0, g_case % 4 < 2);
	}
	// one side in one batch (all of it arrives before the other side's first batch is used up), the other in single records
	for (g_case = 20000; g_case < 20100; ++g_case) {
		const uint64_t n = 1 + rng() % 50;
		std::mt19937_64 r2(g_case);
		MibfZip z;
		uint64_t pairs = 0, fed1 = 0;
		bool big_fed = false;
		for (;;) {
			const MibfZip::Step st = z.step();
			if (st == MibfZip::END)
				break;
			CHECK(st != MibfZip::UNEQUAL);
			if (st == MibfZip::TAKE) {
				CHECK(z.pos(0) == pairs && z.take() == 1);
				++pairs;
			} else if (st == MibfZip::NEED_0) {
				z.feed(0, big_fed ? 0 : n, big_fed);
				big_fed = true;
			} else {
				z.feed(1, fed1 < n ? 1 : 0, fed1 >= n);
				fed1 += fed1 < n;
			}
		}
		CHECK(pairs == n);
	}
	// both sides empty; one side empty
	{
		MibfZip z;
		CHECK(z.step() == MibfZip::NEED_0);
		z.feed(0, 0, true);
		CHECK(z.step() == MibfZip::NEED_1);
		z.feed(1, 0, true);
		CHECK(z.step() == MibfZip::END);
		MibfZip y;
		y.feed(0, 0, true);
		y.feed(1, 1, false);
		CHECK(y.step() == MibfZip::UNEQUAL);
	}
	std::printf("mibf zip test passed\n");
	return 0;
}
