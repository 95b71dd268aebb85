// examples/bloom_merge.cpp -- combine stored filters without reading the data again: what a caller of the reference
// writes as loops over getFilter() on the host, here on the arrays in HBM over the drop-in headers.
//
//   g++ -std=c++17 -O2 -Iinclude examples/bloom_merge.cpp -Lbtl_bloomfilter_amd -lbtlbf \
//       -Wl,-rpath,$PWD/btl_bloomfilter_amd -Wl,-rpath,/opt/rocm/lib -o bloom_merge
//   ./bloom_merge union out.bf lane1.bf lane2.bf lane3.bf     (also: intersect, subtract = the first minus the others)
//   ./bloom_merge fold 8 out.bf in.bf                         the filter an eighth the size that the same data builds
//   ./bloom_merge solid 3 out.bf counts.bf [-w 8|16|32|64]    the bit filter of the k-mers counted at least 3 times
//
// The filters of one union / intersect / subtract (BloomFilter::storeFilter files, up to 17) must share their size, hash
// count and k-mer size.  `solid` reads a CountingBloomFilter<T> file; the file does not record T, so -w gives the
// counter's width in bits (default 8).  Every command prints the result's size, set bits and false-positive rate.
#include "btlbf/BloomFilter.hpp"
#include "btlbf/CountingBloomFilter.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static int usage()
{
	std::fprintf(stderr, "usage: bloom_merge union|intersect|subtract out.bf a.bf b.bf ...\n"
	                     "       bloom_merge fold N out.bf in.bf\n"
	                     "       bloom_merge solid T out.bf counts.bf [-w 8|16|32|64]\n");
	return 2;
}

static int report(BloomFilter& f, const std::string& path)
{
	f.storeFilter(path);
	std::printf("%s\tbits %llu\tset %llu\tFPR %.6g\n", path.c_str(), (unsigned long long)f.getFilterSize(),
	            (unsigned long long)f.getPop(), f.getFPR());
	return 0;
}

template<typename T>
static int solid(const std::string& in, unsigned threshold, const std::string& out)
{
	const CountingBloomFilter<T> counts(in, threshold);
	BloomFilter bits = counts.toBloomFilter(threshold);
	return report(bits, out);
}

int main(int argc, char** argv)
{
	std::vector<std::string> pos;
	unsigned width = 8;
	for (int i = 1; i < argc; ++i) {
		if (!std::strcmp(argv[i], "-w") && i + 1 < argc)
			width = (unsigned)std::strtoul(argv[++i], nullptr, 10);
		else
			pos.push_back(argv[i]);
	}
	if (pos.empty())
		return usage();
	const std::string& cmd = pos[0];
	if (cmd == "union" || cmd == "intersect" || cmd == "subtract") {
		if (pos.size() < 4)
			return usage();
		BloomFilter acc(pos[2]);
		std::vector<std::unique_ptr<BloomFilter> > owned;
		std::vector<const BloomFilter*> others;
		for (size_t i = 3; i < pos.size(); ++i) {
			owned.emplace_back(new BloomFilter(pos[i]));
			others.push_back(owned.back().get());
		}
		if (cmd == "union")
			acc.merge(others);
		else if (cmd == "intersect")
			acc.intersect(others);
		else
			acc.subtract(others);
		return report(acc, pos[1]);
	}
	if (cmd == "fold") {
		if (pos.size() != 4)
			return usage();
		const BloomFilter in(pos[3]);
		BloomFilter out = in.fold(std::strtoull(pos[1].c_str(), nullptr, 10));
		return report(out, pos[2]);
	}
	if (cmd == "solid") {
		if (pos.size() != 4)
			return usage();
		const unsigned t = (unsigned)std::strtoul(pos[1].c_str(), nullptr, 10);
		switch (width) {
		case 8: return solid<uint8_t>(pos[3], t, pos[2]);
		case 16: return solid<uint16_t>(pos[3], t, pos[2]);
		case 32: return solid<uint32_t>(pos[3], t, pos[2]);
		case 64: return solid<uint64_t>(pos[3], t, pos[2]);
		default: return usage();
		}
	}
	return usage();
}
