// tests/cpp/ref_mibf_classify_pair_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// The genuine reference's classification of read PAIRS, for tests/test_mibf_classify_pairs_vs_ref.py; it follows
// tests/cpp/ref_mibf_classify_driver.cpp (same input format, include order and m_extraCount handling) with the queries
// taken two by two: query 2i is mate 1 and query 2i + 1 mate 2 of pair i.  A program around the reference's
// MIBFConstructSupport.hpp and MIBFQuerySupport.hpp, compiled by the test from where those headers lie (never copied
// here) over the stand-ins of oracle/standin/ (sdsl, sparsehash) and tests/cpp/standin/ (boost's binomial).
// It builds a miBF from the test's sequences (insertBV, getEmptyMIBF, insertMIBF, insertSaturation) and runs
// MIBFQuerySupport<T>::query(itr1, itr2, minCount) on the pairs for every parameter set.
//
// Include order as in oracle/ref_mibf_driver.cpp: MIBloomFilter.hpp sets `#pragma pack(1)` and never resets it, so
// every standard and vendor header comes first and the packing is reset behind the reference headers.
//
// extra_count: the reference's constructor takes `unsigned extraCount` and stores it in `const double m_extraCount`,
// so a fraction cannot pass through it.  The member is what the comparisons use; the driver (built with
// -fno-access-control) sets it behind the constructor, from a value read at run time.
//
// Input (a text file, argv[1]); an empty sequence is written as "-":
//   id_bytes k h n_seeds [seed ...] expected_entries occupancy
//   n_insert, then per line: id sequence
//   n_ids, then per id: per_frame_prob min_count
//   n_params, then per line: extra_count extra_frame_limit max_miss min_count best_hit_agree
//   n_queries (even), then one sequence per line
// Output: "size <bits> <pop>", "data <pop values>", then per (parameter set p, pair q)
//   "r p q satCount evalCount evalCountWithoutStop n {id count nonSatCount totalCount totalNonSatCount nonSatFrameCount solidCount}*n"
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
#include "MIBFQuerySupport.hpp"
#pragma pack()

namespace {

struct Params
{
	double extra_count;
	unsigned extra_frame_limit, max_miss, min_count, best_hit_agree;
};

struct Input
{
	unsigned id_bytes, k, h;
	std::vector<std::string> seeds;
	size_t entries;
	double occupancy;
	std::vector<std::pair<unsigned, std::string> > inserts;
	std::vector<double> prob;
	std::vector<unsigned> min_count;
	std::vector<Params> params;
	std::vector<std::string> queries;
};

std::string
seq_of(const std::string& s)
{
	return s == "-" ? std::string() : s;
}

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
__attribute__((noinline)) MIBFQuerySupport<T>*
make_support(const MIBloomFilter<T>& mi, const Input& in, const Params& p, unsigned limit)
{
	MIBFQuerySupport<T>* qs = new MIBFQuerySupport<T>(
	    mi, in.prob, (unsigned)p.extra_count, limit, p.max_miss, p.min_count, p.best_hit_agree != 0);
	volatile double e = p.extra_count;
	const_cast<double&>(qs->m_extraCount) = e;
	return qs;
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
	printf("size %llu %llu\ndata", (unsigned long long)mi->size(), (unsigned long long)mi->getPop());
	for (size_t r = 0; r < mi->getPop(); ++r)
		printf(" %u", (unsigned)mi->getData(r));
	printf("\n");
	for (size_t pi = 0; pi < in.params.size(); ++pi) {
		const Params& p = in.params[pi];
		MIBFQuerySupport<T>* qs = make_support<T, H>(*mi, in, p, p.extra_frame_limit);
		MIBFQuerySupport<T>* full = make_support<T, H>(*mi, in, p, 0xffffffffu);
		for (size_t qi = 0; qi < in.queries.size() / 2; ++qi) {
			H* a = make(in, parsed, in.queries[2 * qi], (H*)NULL);
			H* b = make(in, parsed, in.queries[2 * qi + 1], (H*)NULL);
			full->query(*a, *b, in.min_count);
			const unsigned eval_full = full->getEvalCount();
			delete a;
			delete b;
			a = make(in, parsed, in.queries[2 * qi], (H*)NULL);
			b = make(in, parsed, in.queries[2 * qi + 1], (H*)NULL);
			const std::vector<typename MIBFQuerySupport<T>::QueryResult>& res = qs->query(*a, *b, in.min_count);
			delete a;
			delete b;
			printf("r %zu %zu %u %u %u %zu", pi, qi, qs->getSatCount(), qs->getEvalCount(), eval_full, res.size());
			for (size_t i = 0; i < res.size(); ++i) {
				if (res[i].frameProb != in.prob[res[i].id])
					return 3;
				printf(" %u %u %u %u %u %u %u", (unsigned)res[i].id, res[i].count, res[i].nonSatCount, res[i].totalCount,
				       res[i].totalNonSatCount, res[i].nonSatFrameCount, res[i].solidCount);
			}
			printf("\n");
		}
		delete qs;
		delete full;
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
	for (size_t i = 0; i < n; ++i) {
		f >> in.inserts[i].first >> in.inserts[i].second;
		in.inserts[i].second = seq_of(in.inserts[i].second);
	}
	f >> n;
	in.prob.resize(n);
	in.min_count.resize(n);
	for (size_t i = 0; i < n; ++i)
		f >> in.prob[i] >> in.min_count[i];
	f >> n;
	in.params.resize(n);
	for (size_t i = 0; i < n; ++i)
		f >> in.params[i].extra_count >> in.params[i].extra_frame_limit >> in.params[i].max_miss >>
		    in.params[i].min_count >> in.params[i].best_hit_agree;
	f >> n;
	in.queries.resize(n);
	for (size_t i = 0; i < n; ++i) {
		f >> in.queries[i];
		in.queries[i] = seq_of(in.queries[i]);
	}
	if (!f || in.queries.size() % 2)
		return 2;
	const bool seeded = !in.seeds.empty();
	if (in.id_bytes == 2)
		return seeded ? run<uint16_t, stHashIterator>(in) : run<uint16_t, ntHashIterator>(in);
	return seeded ? run<uint32_t, stHashIterator>(in) : run<uint32_t, ntHashIterator>(in);
}
