// tests/cpp/ref_mibf_frame_probs_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// The genuine reference's calcFrameProbs, for tests/test_mibf_frame_probs_vs_ref.py: a program around the reference's
// MIBFConstructSupport.hpp and MIBloomFilter.hpp, compiled by the test from where those headers lie (never copied here)
// over the stand-ins of oracle/standin/ and tests/cpp/standin/, as tests/cpp/ref_mibf_classify_driver.cpp is.  It builds
// the miBF of the test's sequences (insertBV, getEmptyMIBF, insertMIBF, insertSaturation) and prints
// MIBloomFilter<T>::calcFrameProbs(frameProbs, allowedMiss) for every allowedMiss below the hash count.
//
// Include order as in oracle/ref_mibf_driver.cpp: MIBloomFilter.hpp sets `#pragma pack(1)` and never resets it, so
// every standard and vendor header comes first and the packing is reset behind the reference headers.
//
// Input (a text file, argv[1]); the head of ref_mibf_classify_driver.cpp's:
//   id_bytes k h n_seeds [seed ...] expected_entries occupancy
//   n_insert, then per line: id sequence
//   n_bins                         (frameProbs.size(): the largest id + 1)
// Output: "size <bits> <pop>", "counts <saturated> <n_bins values of getIDCounts>", then per allowedMiss a
//   "p a <satProp> <frameProbs[1]> ... <frameProbs[n_bins - 1]>" as hex floats; frameProbs[0] is checked to be untouched.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <random>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include <boost/math/distributions/binomial.hpp>

#include "vendor/ntHashIterator.hpp"
#include "vendor/stHashIterator.hpp"

#include "MIBFConstructSupport.hpp"
#pragma pack()

namespace {

struct Input
{
	unsigned id_bytes, k, h;
	std::vector<std::string> seeds;
	size_t entries, n_bins;
	double occupancy;
	std::vector<std::pair<unsigned, std::string> > inserts;
};

ntHashIterator*
make(const Input& in, const std::vector<std::vector<unsigned> >&, const std::string& s, ntHashIterator*)
{
	return new ntHashIterator(s, in.h, in.k);
}
stHashIterator*
make(const Input& in, const std::vector<std::vector<unsigned> >& parsed, const std::string& s, stHashIterator*)
{
	return new stHashIterator(s, parsed, in.h, 1, in.k);
}

template<typename T, class H>
int
run(const Input& in)
{
	const std::vector<std::vector<unsigned> > parsed = stHashIterator::parseSeed(in.seeds);
	MIBFConstructSupport<T, H> cs(in.entries, in.k, in.h, in.occupancy, in.seeds);
	for (size_t i = 0; i < in.inserts.size(); ++i) {
		H* it = make(in, parsed, in.inserts[i].second, (H*)NULL);
		cs.insertBV(*it);
		delete it;
	}
	MIBloomFilter<T>* mi = cs.getEmptyMIBF();
	for (size_t i = 0; i < in.inserts.size(); ++i) {
		H* it = make(in, parsed, in.inserts[i].second, (H*)NULL);
		cs.insertMIBF(*mi, *it, (T)in.inserts[i].first);
		delete it;
	}
	for (size_t i = 0; i < in.inserts.size(); ++i) {
		H* it = make(in, parsed, in.inserts[i].second, (H*)NULL);
		cs.insertSaturation(*mi, *it, (T)in.inserts[i].first);
		delete it;
	}
	printf("size %llu %llu\n", (unsigned long long)mi->size(), (unsigned long long)mi->getPop());
	std::vector<size_t> counts(in.n_bins, 0);
	const size_t sat = mi->getIDCounts(counts);
	printf("counts %zu", sat);
	for (size_t i = 0; i < counts.size(); ++i)
		printf(" %zu", counts[i]);
	printf("\n");
	for (unsigned a = 0; a < in.h; ++a) {
		std::vector<double> probs(in.n_bins, -7.5);
		const double sat_prop = mi->calcFrameProbs(probs, a);
		if (probs[0] != -7.5)
			return 3;
		printf("p %u %a", a, sat_prop);
		for (size_t i = 1; i < probs.size(); ++i)
			printf(" %a", probs[i]);
		printf("\n");
	}
	delete mi;
	return 0;
}

} // namespace

int
main(int argc, char** argv)
{
	if (argc != 2)
		return 2;
	std::ifstream f(argv[1]);
	Input in;
	size_t n;
	f >> in.id_bytes >> in.k >> in.h >> n;
	in.seeds.resize(n);
	for (size_t i = 0; i < n; ++i)
		f >> in.seeds[i];
	f >> in.entries >> in.occupancy >> n;
	in.inserts.resize(n);
	for (size_t i = 0; i < n; ++i)
		f >> in.inserts[i].first >> in.inserts[i].second;
	f >> in.n_bins;
	if (!f)
		return 2;
	const bool seeded = !in.seeds.empty();
	if (in.id_bytes == 2)
		return seeded ? run<uint16_t, stHashIterator>(in) : run<uint16_t, ntHashIterator>(in);
	return seeded ? run<uint32_t, stHashIterator>(in) : run<uint32_t, ntHashIterator>(in);
}
