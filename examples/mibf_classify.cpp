// examples/mibf_classify.cpp -- classify the reads of one or two FASTA / FASTQ files (plain or gzip) against a stored
// multi-index Bloom filter: what a caller of the reference writes around MIBloomFilter<T>::calcFrameProbs and
// MIBFQuerySupport<T>::query, here as three calls over the drop-in headers.
//
//   g++ -std=c++17 -O2 -Iinclude examples/mibf_classify.cpp -Lbtl_bloomfilter_amd -lbtlbf \
//       -Wl,-rpath,$PWD/btl_bloomfilter_amd -Wl,-rpath,/opt/rocm/lib -o mibf_classify
//   ./mibf_classify stage1.bf ids.mibf 41 reads_1.fq.gz reads_2.fq.gz          # pairs from two files, ids 1..40
//   ./mibf_classify stage1.bf ids.mibf 41 reads.fq --interleaved --max-miss 1
//
// stage1.bf is the bit filter the miBF was built on (BloomFilter::storeFilter), ids.mibf the ID array
// (MIBloomFilter::store; its header carries the spaced seeds), the number is the size of the per-id tables (largest
// id + 1).  Output: one line `row<TAB>id<TAB>count<TAB>nonSatFrameCount` per result, rows (records, or pairs) in file
// order, then `#id<TAB>best<TAB>any` per id with a row and a `#totals` line.  Options: --u32 (uint32_t ids),
// --interleaved, --max-miss N, --allowed-miss N (calcFrameProbs; default: max-miss), --min-count N (minCount of every id),
// --min-frames N, --extra-count X, --extra-frame-limit N, --best-hit-agree, --max-results N, --batch-bytes N.
#include "btlbf/MIBFQuerySupport.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct Options {
	std::string stage1, data, reads1, reads2;
	size_t nIds = 0;
	bool u32 = false, interleaved = false, bestHitAgree = false;
	unsigned maxMiss = 0, minCount = 1, minFrames = 1, extraFrameLimit = 0, maxResults = 8;
	int allowedMiss = -1;
	double extraCount = 1.0;
	uint64_t batchBytes = 0;
};

template<typename T>
static int run(const Options& o)
{
	btlbf_filter* bf = nullptr;
	btlbf_shim::check(btlbf_load(&bf, BTLBF_BLOOM, o.stage1.c_str(), 0, 0));
	btlbf::MIBloomFilter<T> miBF(o.data, bf);
	btlbf_destroy(bf);
	std::vector<double> perFrameProb(o.nIds, 0.0);
	const double satProp = miBF.calcFrameProbs(perFrameProb, o.allowedMiss < 0 ? o.maxMiss : (unsigned)o.allowedMiss);
	const std::vector<unsigned> minCount(o.nIds, o.minCount);
	btlbf::MIBFQuerySupport<T> support(miBF, perFrameProb, o.extraCount, o.extraFrameLimit, o.maxMiss, o.minFrames,
	                                   o.bestHitAgree, o.maxResults);
	typedef typename btlbf::MIBFQuerySupport<T>::QueryResult Result;
	std::vector<uint64_t> best(o.nIds, 0), any(o.nIds, 0);
	uint64_t without = 0;
	auto sink = [&](uint64_t firstRow, const std::vector<std::vector<Result> >& results, const std::vector<uint32_t>&,
	                const std::vector<uint32_t>&) {
		for (size_t r = 0; r < results.size(); ++r) {
			without += results[r].empty();
			for (size_t i = 0; i < results[r].size(); ++i) {
				const Result& q = results[r][i];
				std::printf("%llu\t%u\t%u\t%u\n", (unsigned long long)(firstRow + r), (unsigned)q.id, (unsigned)q.count,
				            (unsigned)q.nonSatFrameCount);
				++any[q.id];
				if (i == 0)
					++best[q.id];
			}
		}
	};
	const uint64_t rows = !o.reads2.empty() ? support.queryFiles(o.reads1, o.reads2, minCount, sink, o.batchBytes)
	                      : o.interleaved   ? support.queryInterleavedFile(o.reads1, minCount, sink, o.batchBytes)
	                                        : support.queryFile(o.reads1, minCount, sink, o.batchBytes);
	for (size_t i = 0; i < o.nIds; ++i)
		if (any[i])
			std::printf("#%zu\t%llu\t%llu\n", i, (unsigned long long)best[i], (unsigned long long)any[i]);
	std::printf("#totals\trows %llu\twithout a result %llu\tsaturated entries %.6g\n", (unsigned long long)rows,
	            (unsigned long long)without, satProp);
	return 0;
}

static int usage()
{
	std::fprintf(stderr, "usage: mibf_classify <stage1.bf> <ids.mibf> <n_ids> <reads_1> [reads_2] [--u32] [--interleaved]\n"
	                     "         [--max-miss N] [--allowed-miss N] [--min-count N] [--min-frames N] [--extra-count X]\n"
	                     "         [--extra-frame-limit N] [--best-hit-agree] [--max-results N] [--batch-bytes N]\n");
	return 2;
}

int main(int argc, char** argv)
{
	Options o;
	std::vector<std::string> pos;
	for (int i = 1; i < argc; ++i) {
		const std::string a = argv[i];
		auto value = [&]() -> const char* { return i + 1 < argc ? argv[++i] : "0"; };
		if (a == "--u32")
			o.u32 = true;
		else if (a == "--interleaved")
			o.interleaved = true;
		else if (a == "--best-hit-agree")
			o.bestHitAgree = true;
		else if (a == "--max-miss")
			o.maxMiss = (unsigned)std::atoi(value());
		else if (a == "--allowed-miss")
			o.allowedMiss = std::atoi(value());
		else if (a == "--min-count")
			o.minCount = (unsigned)std::atoi(value());
		else if (a == "--min-frames")
			o.minFrames = (unsigned)std::atoi(value());
		else if (a == "--extra-count")
			o.extraCount = std::atof(value());
		else if (a == "--extra-frame-limit")
			o.extraFrameLimit = (unsigned)std::strtoul(value(), nullptr, 10);
		else if (a == "--max-results")
			o.maxResults = (unsigned)std::atoi(value());
		else if (a == "--batch-bytes")
			o.batchBytes = std::strtoull(value(), nullptr, 10);
		else if (a.size() > 1 && a[0] == '-' && a[1] == '-')
			return usage();
		else
			pos.push_back(a);
	}
	if (pos.size() < 4 || pos.size() > 5 || (pos.size() == 5 && o.interleaved))
		return usage();
	o.stage1 = pos[0];
	o.data = pos[1];
	o.nIds = (size_t)std::strtoull(pos[2].c_str(), nullptr, 10);
	o.reads1 = pos[3];
	if (pos.size() == 5)
		o.reads2 = pos[4];
	return o.u32 ? run<uint32_t>(o) : run<uint16_t>(o);
}
