// examples/bloom_size.cpp -- how large must the Bloom filter for these reads be?
//
//   bloom_size [-k K] [-s S] [-r R] [-p fpr] [-g H] [-t T] reads.fq[.gz] ...
//
// Estimates the distinct k-mers of the files (F0) and their abundance spectrum (f1, f2, ...) with btlbf::KmerCardinality
// -- one pass over the reads on the GPU, a sketch of 4 << R bytes -- and prints the bit count
// BloomFilter::calcOptimalSize(F0, fpr, H) a filter of all of them needs.  With -t T it prints the same for the k-mers
// seen at least T times: what CountingBloomFilter::toBloomFilter(T) of a counting filter over these reads would hold.
//   -k k-mer size (31)   -s sample bits (11: one window in 2048)   -r table bits (22)
//   -p false positive rate (0.01)   -g hash functions (0: the optimum for -p)   -t abundance threshold (none)
#include <btlbf/BloomFilter.hpp>
#include <btlbf/KmerCardinality.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int usage()
{
	std::fprintf(stderr, "usage: bloom_size [-k K] [-s S] [-r R] [-p fpr] [-g H] [-t T] reads.fq[.gz] ...\n");
	return 2;
}

int main(int argc, char** argv)
{
	unsigned k = 31, s = btlbf::KmerCardinality::kDefaultSampleBits, r = btlbf::KmerCardinality::kDefaultTableBits, h = 0, t = 0;
	double fpr = 0.01;
	std::vector<std::string> paths;
	for (int i = 1; i < argc; ++i) {
		const char* a = argv[i];
		if (a[0] == '-' && a[1] && !a[2] && std::strchr("ksrpgt", a[1])) {
			if (++i >= argc)
				return usage();
			switch (a[1]) {
			case 'k': k = (unsigned)std::atoi(argv[i]); break;
			case 's': s = (unsigned)std::atoi(argv[i]); break;
			case 'r': r = (unsigned)std::atoi(argv[i]); break;
			case 'p': fpr = std::atof(argv[i]); break;
			case 'g': h = (unsigned)std::atoi(argv[i]); break;
			default: t = (unsigned)std::atoi(argv[i]); break;
			}
		} else if (a[0] == '-') {
			return usage();
		} else {
			paths.push_back(a);
		}
	}
	if (paths.empty() || !(fpr > 0.0 && fpr < 1.0))
		return usage();
	if (h == 0)
		h = BloomFilter::calcOptiHashNum(fpr);
	if (h == 0)
		h = 1;

	btlbf::KmerCardinality card(k, s, r);
	uint64_t records = 0;
	for (size_t i = 0; i < paths.size(); ++i)
		records += card.addFile(paths[i]).n_records;
	const unsigned nHist = t + 2 > 16 ? t + 2 : 16;
	const btlbf::KmerCardinality::Estimate e = card.estimate(nHist);

	std::printf("records\t%llu\nkmers\t%llu\nsampled\t%llu\n", (unsigned long long)records, (unsigned long long)e.cleanWindows,
	            (unsigned long long)e.sampled);
	std::printf("F0\t%.17g\nf1\t%.17g\n", e.distinct, e.singletons);
	for (size_t i = 2; i < e.spectrum.size() && i <= 8; ++i)
		std::printf("f%zu\t%.17g\n", i, e.spectrum[i]);
	std::printf("occupancy\t%.6f%s\n", e.occupancy,
	            e.occupancy < 0.05   ? "\t(low: lower -s or -r for a tighter estimate)"
	            : e.occupancy > 0.8 ? "\t(high: raise -r or -s)"
	                                : "");
	std::printf("bits\t%zu\t(F0 k-mers, fpr %g, %u hash functions)\n", BloomFilter::calcOptimalSize((size_t)e.distinct, fpr, h), fpr,
	            h);
	if (t) {
		const double solid = e.atLeast(t) > 0 ? e.atLeast(t) : 0;
		std::printf("F0_at_least_%u\t%.17g\nbits_at_least_%u\t%zu\n", t, solid, t, BloomFilter::calcOptimalSize((size_t)solid, fpr, h));
	}
	return 0;
}
