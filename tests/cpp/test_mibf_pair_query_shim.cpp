// tests/cpp/test_mibf_pair_query_shim.cpp -- the paired calls of btlbf::MIBFQuerySupport<T>
// (include/btlbf/MIBFQuerySupport.hpp) on the input file of tests/cpp/ref_mibf_classify_pair_driver.cpp, answering in that
// driver's output format: the miBF is built through the C ABI and the MIBloomFilter shim (serial saturation, as the
// reference), the queries are taken two by two as the mates of a pair, every pair runs through query(seq1, seq2, ...)
// and through queryPairs, and the two must agree.  tests/test_gpu_cpp_mibf_pair_query.py compares the output with the
// pinned model.  argv: input file.  The filter has the size the reference's constructor computes
// (MIBloomFilter.hpp:84-88).
#define BTLBF_SHIM_THROW // errors as exceptions: the unequal-sizes case below is caught
#include <btlbf/MIBFQuerySupport.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <string>
#include <vector>

template<typename T>
static int
run(std::ifstream& f, unsigned k, unsigned h, const std::vector<std::string>& seeds, uint64_t bits)
{
	size_t n;
	f >> n;
	std::vector<uint32_t> ids(n);
	std::string all;
	unsigned len = 0;
	for (size_t i = 0; i < n; ++i) {
		std::string s;
		f >> ids[i] >> s;
		if (len && s.size() != len)
			return 4; // the shim's insertIDs takes reads of one length
		len = s.size();
		all += s;
	}
	btlbf_filter* bf = nullptr;
	btlbf_shim::check(btlbf_create(&bf, BTLBF_BLOOM, bits, h, k, 0, 0));
	if (!seeds.empty()) {
		std::vector<const char*> sp;
		for (size_t i = 0; i < seeds.size(); ++i)
			sp.push_back(seeds[i].c_str());
		btlbf_shim::check(btlbf_set_spaced_seeds(bf, &sp[0], sp.size(), 1));
	}
	btlbf_layout l = {nullptr, 0, len};
	btlbf_shim::check(btlbf_insert_seqs(bf, all.data(), all.size(), &l, BTLBF_INCREMENT_MIN, BTLBF_ORDER_PARALLEL, BTLBF_HOST, nullptr));
	btlbf::MIBloomFilter<T> mi(bf);
	btlbf_destroy(bf);
	mi.insertIDs(all, len, ids);
	mi.insertSaturation(all, len, ids, true);
	f >> n;
	std::vector<double> prob(n);
	std::vector<unsigned> minc(n);
	for (size_t i = 0; i < n; ++i)
		f >> prob[i] >> minc[i];
	size_t np;
	f >> np;
	std::vector<std::vector<double> > par(np, std::vector<double>(5));
	for (size_t i = 0; i < np; ++i)
		for (int j = 0; j < 5; ++j)
			f >> par[i][j];
	f >> n;
	std::vector<std::string> q(n);
	for (size_t i = 0; i < n; ++i) {
		f >> q[i];
		if (q[i] == "-")
			q[i].clear();
	}
	if (!f || n % 2)
		return 2;
	std::vector<std::string> q1, q2;
	for (size_t i = 0; i < n; i += 2) {
		q1.push_back(q[i]);
		q2.push_back(q[i + 1]);
	}
	printf("size %llu %llu\ndata", (unsigned long long)mi.size(), (unsigned long long)mi.getPop());
	const std::vector<T> d = mi.getData();
	for (size_t i = 0; i < d.size(); ++i)
		printf(" %u", (unsigned)d[i]);
	printf("\n");
	for (size_t pi = 0; pi < np; ++pi) {
		btlbf::MIBFQuerySupport<T> qs(mi, prob, par[pi][0], (unsigned)par[pi][1], (unsigned)par[pi][2], (unsigned)par[pi][3],
		                              par[pi][4] != 0);
		const typename btlbf::MIBFQuerySupport<T>::BatchResult b = qs.queryPairs(q1, q2, minc);
		if (b.results.size() != q1.size())
			return 5;
		for (size_t qi = 0; qi < q1.size(); ++qi) {
			const std::vector<typename btlbf::MIBFQuerySupport<T>::QueryResult>& r = qs.query(q1[qi], q2[qi], minc);
			if (r.size() != b.results[qi].size() || qs.getSatCount() != b.satCount[qi] || qs.getEvalCount() != b.evalCount[qi] ||
			    b.nResults[qi] != r.size())
				return 5;
			printf("r %zu %zu %u %u %u %zu", pi, qi, qs.getSatCount(), qs.getEvalCount(), 0u, r.size());
			for (size_t i = 0; i < r.size(); ++i) {
				const typename btlbf::MIBFQuerySupport<T>::QueryResult& x = r[i];
				const typename btlbf::MIBFQuerySupport<T>::QueryResult& y = b.results[qi][i];
				if (x.id != y.id || x.count != y.count || x.totalCount != y.totalCount || x.frameProb != prob[x.id])
					return 5;
				printf(" %u %u %u %u %u %u %u", (unsigned)x.id, x.count, x.nonSatCount, x.totalCount, x.totalNonSatCount,
				       x.nonSatFrameCount, x.solidCount);
			}
			printf("\n");
		}
	}
	// mates that do not pair up are refused before anything runs
	btlbf::MIBFQuerySupport<T> qs(mi, prob, 1.0, 0, 0, 1, false);
	q2.pop_back();
	try {
		qs.queryPairs(q1, q2, minc);
		return 6;
	} catch (const std::exception&) {
	}
	return 0;
}

int
main(int argc, char** argv)
{
	if (argc != 2)
		return 2;
	std::ifstream f(argv[1]);
	unsigned id_bytes, k, h;
	size_t ns;
	f >> id_bytes >> k >> h >> ns;
	std::vector<std::string> seeds(ns);
	for (size_t i = 0; i < ns; ++i)
		f >> seeds[i];
	size_t entries;
	double occ;
	f >> entries >> occ;
	uint64_t bits = (uint64_t)(-(double)entries * (double)h / log(1.0 - occ));
	bits += 64 - bits % 64;
	return id_bytes == 2 ? run<uint16_t>(f, k, h, seeds, bits) : run<uint32_t>(f, k, h, seeds, bits);
}
