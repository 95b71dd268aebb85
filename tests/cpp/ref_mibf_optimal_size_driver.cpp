// tests/cpp/ref_mibf_optimal_size_driver.cpp -- TEST-ONLY: the genuine MIBloomFilter<T>::calcOptimalSize
// (MIBloomFilter.hpp:84-88) of the reference tree, the function MIBFConstructSupport's constructor sizes its bit vector
// with, for `entries hashNum occupancy` triples given as arguments: one size per line.  The constructor itself cannot
// be asked at 2^40 entries: it allocates the bit vector.  Built by tests/test_mibf_build_size_vs_ref.py where the
// reference tree lies.
#include <algorithm>
#include <random> // the reference header uses std::minstd_rand without including it

#include "MIBloomFilter.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
	for (int i = 1; i + 2 < argc; i += 3) {
		const size_t entries = std::strtoull(argv[i], nullptr, 10);
		const unsigned h = (unsigned)std::atoi(argv[i + 1]);
		const double occ = std::strtod(argv[i + 2], nullptr);
		std::printf("%llu\n", (unsigned long long)MIBloomFilter<uint16_t>::calcOptimalSize(entries, h, occ));
	}
	return 0;
}
