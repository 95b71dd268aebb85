// tests/cpp/test_shims_wide.cpp -- the reference's counting-filter unit test (Tests/Unit/CountingBloomFilterTests.cpp:
// the common setup, "query elements", "save/load 64 bit Bloom file") for T = uint64_t and T = uint16_t, written against
// the drop-in shim include/btlbf/CountingBloomFilter.hpp, plus what a counter wider than a byte is for: counts above
// 255 through operator[] and minCount.  A user of the reference changes only the include paths.  Needs a GPU.
#include "btlbf/CountingBloomFilter.hpp"
#include "btlbf/ntHashIterator.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <unistd.h>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                    \
	do {                                                                               \
		if (!(cond)) {                                                                 \
			std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
			++g_fail;                                                                  \
		}                                                                              \
	} while (0)

template<typename T>
static void reference_unit_test(const char* tag)
{
	const size_t filterSize = 100001;
	const unsigned numHashes = 5, threshold = 1, k = 8;
	const char* seq = "ACGTACACTGGACTGAGTCT";
	CountingBloomFilter<T> filter(filterSize, numHashes, k, threshold);
	CHECK(filter.sizeInBytes() == 100008 && filter.size() * sizeof(T) == filter.sizeInBytes());
	ntHashIterator insertIt(seq, numHashes, k);
	while (insertIt != insertIt.end()) {
		filter.insert(*insertIt);
		++insertIt;
	}
	// "query elements"
	ntHashIterator queryIt(seq, numHashes, k);
	unsigned n = 0;
	while (queryIt != queryIt.end()) {
		CHECK(filter.contains(*queryIt));
		CHECK(filter.minCount(*queryIt) >= 1);
		++queryIt;
		++n;
	}
	CHECK(n == 13);
	const std::string other = "TTGACCAGTTACGGATCCAGTAGGCATTAGCCATGATCGGGATACCATGAACTTGACTGA";
	ntHashIterator o(other, numHashes, k);
	while (o != o.end()) {
		CHECK(!filter.contains(*o));
		++o;
	}
	// "save/load <bits> bit Bloom file"
	char fn[256];
	std::snprintf(fn, sizeof fn, "/tmp/btlbf_shim_wide_%s_%d.bf", tag, (int)getpid());
	filter.storeFilter(fn);
	std::ifstream ifile(fn);
	CHECK(ifile.is_open());
	std::string line;
	bool headerEndCheck = false;
	while (std::getline(ifile, line))
		if (line == "[HeaderEnd]") {
			headerEndCheck = true;
			break;
		}
	CHECK(headerEndCheck);
	const size_t currPos = ifile.tellg();
	ifile.seekg(0, std::ios::end);
	const size_t endPos = ifile.tellg();
	CHECK(endPos - currPos == filterSize + 8 - filterSize % 8);
	ifile.close();
	CountingBloomFilter<T> filter2(fn, threshold);
	CHECK(endPos - currPos == filter2.sizeInBytes());
	CHECK(filter2.size() * sizeof(T) == filter2.sizeInBytes());
	CHECK(filter2.popCount() == filter.popCount() && filter2.filtered_popcount() == filter.filtered_popcount());
	ntHashIterator q2(seq, numHashes, k);
	while (q2 != q2.end()) {
		CHECK(filter2.contains(*q2));
		++q2;
	}
	std::remove(fn);

	// counts a byte cannot hold: 300 x incrementAll of one row; positions are hash % size() -- the counter count
	const uint64_t size = filter.size();
	std::vector<uint64_t> hv = {1, size + 1, 2, 3, 4}; // counters 1, 1, 2, 3, 4
	for (int i = 0; i < 300; ++i)
		filter.incrementAll(hv);
	CHECK(filter[1] >= 600 && filter[2] >= 300 && filter[2] < 600);
	CHECK(filter.minCount(hv) >= 300 && filter.minCount(hv) == std::min<T>(filter[2], std::min<T>(filter[3], filter[4])));
	CHECK(filter.insertAndCheck(hv));
	CountingBloomFilter<T> strict(64, 2, k, 256);
	std::vector<uint64_t> two = {3, 5};
	for (int i = 0; i < 255; ++i)
		strict.insert(two);
	CHECK(!strict.contains(two) && strict.minCount(two) == 255);
	strict.insert(two);
	CHECK(strict.contains(two) && strict.minCount(two) == 256 && strict[3] == 256 && strict[5] == 256);
}

int main()
{
	reference_unit_test<uint64_t>("u64");
	reference_unit_test<uint16_t>("u16");
	reference_unit_test<uint32_t>("u32");
	if (g_fail) {
		std::printf("%d wide shim checks failed\n", g_fail);
		return 1;
	}
	std::printf("all wide shim tests passed\n");
	return 0;
}
