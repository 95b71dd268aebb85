// tests/cpp/test_mibf_file_shim.cpp -- the file members of the C++ layer (include/btlbf/MIBloomFilter.hpp,
// MIBFQuerySupport.hpp) for tests/test_gpu_cpp_mibf_classify_file.py: loads a stage-1 filter and a miBF data file, prints
// calcFrameProbs as hex floats, the whole-file summary of summarizeFile, and the rows queryInterleavedFile / queryFile
// deliver (their count and a checksum over every field), so that the Python side can compare all of it.
// argv: stage1.bf ids.mibf n_ids max_miss reads_1 reads_2 interleaved.fq
#define BTLBF_SHIM_THROW
#include <btlbf/MIBFQuerySupport.hpp>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

typedef btlbf::MIBFQuerySupport<uint16_t> Support;

struct Rows {
	uint64_t rows = 0, next = 0, sum = 0;
	bool contiguous = true;
	void operator()(uint64_t first, std::vector<std::vector<Support::QueryResult> >& res, const std::vector<uint32_t>& sat,
	                const std::vector<uint32_t>& ev)
	{
		contiguous = contiguous && first == next && sat.size() == res.size() && ev.size() == res.size();
		next = first + res.size();
		rows += res.size();
		for (size_t r = 0; r < res.size(); ++r) {
			sum = sum * 1000003 + sat[r] * 31 + ev[r];
			for (size_t i = 0; i < res[r].size(); ++i) {
				const Support::QueryResult& q = res[r][i];
				sum = sum * 1000003 + q.id + 7 * q.count + 11 * q.nonSatCount + 13 * q.totalCount + 17 * q.totalNonSatCount +
				      19 * q.nonSatFrameCount + 23 * q.solidCount;
			}
		}
	}
};

int main(int argc, char** argv)
{
	if (argc != 8)
		return 2;
	try {
		btlbf_filter* bf = nullptr;
		btlbf_shim::check(btlbf_load(&bf, BTLBF_BLOOM, argv[1], 0, 0));
		btlbf::MIBloomFilter<uint16_t> mi(argv[2], bf);
		btlbf_destroy(bf);
		const size_t n = std::strtoull(argv[3], nullptr, 10);
		const unsigned maxMiss = (unsigned)std::atoi(argv[4]);
		std::vector<double> prob(n, -1.0);
		const double satProp = mi.calcFrameProbs(prob, maxMiss);
		std::printf("probs %a", satProp);
		for (size_t i = 0; i < n; ++i)
			std::printf(" %a", prob[i]);
		std::printf("\nsingle %a\n", btlbf::MIBloomFilter<uint16_t>::calcProbSingleFrame(0.25, 4, 0.125, 1));
		prob[0] = 0.0;
		const std::vector<unsigned> minc(n, 1);
		Support qs(mi, prob, 1.0, 2, maxMiss, 1, false, 3);
		const Support::FileSummary s = qs.summarizeFile(argv[5], argv[6], minc, false, 300);
		std::printf("best");
		for (size_t i = 0; i < n; ++i)
			std::printf(" %llu", (unsigned long long)s.best[i]);
		std::printf("\nany");
		for (size_t i = 0; i < n; ++i)
			std::printf(" %llu", (unsigned long long)s.any[i]);
		std::printf("\ntotals %llu %llu %llu %llu %llu %llu\n", (unsigned long long)s.rows,
		            (unsigned long long)s.rowsWithoutResult, (unsigned long long)s.rowsWithSeveral,
		            (unsigned long long)s.rowsTruncated, (unsigned long long)s.satCount, (unsigned long long)s.evalCount);
		Rows two, il, single;
		const uint64_t r2 = qs.queryFiles(argv[5], argv[6], minc, two, 300);
		const uint64_t ri = qs.queryInterleavedFile(argv[7], minc, il, 300);
		const uint64_t r1 = qs.queryFile(argv[7], minc, single, 300);
		std::printf("two %llu %d %llu\ninterleaved %llu %d %llu\nsingle_rows %llu %d\n", (unsigned long long)r2,
		            (int)two.contiguous, (unsigned long long)two.sum, (unsigned long long)ri, (int)il.contiguous,
		            (unsigned long long)il.sum, (unsigned long long)r1, (int)single.contiguous);
		// the two pairing modes at once are refused
		try {
			qs.summarizeFile(argv[5], argv[6], minc, true, 300);
			return 5;
		} catch (const std::exception&) {
		}
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 3;
	}
	return 0;
}
