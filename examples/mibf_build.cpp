// examples/mibf_build.cpp -- build a multi-index Bloom filter from reference sequences in FASTA / FASTQ files (plain or
// gzip): what a caller of the reference writes around MIBFConstructSupport (count, size the bit vector, insert, rank,
// insert ids, saturate), here as one call over the drop-in headers.  Its output is what examples/mibf_classify.cpp reads.
//
//   g++ -std=c++17 -O2 -Iinclude examples/mibf_build.cpp -Lbtl_bloomfilter_amd -lbtlbf \
//       -Wl,-rpath,$PWD/btl_bloomfilter_amd -Wl,-rpath,/opt/rocm/lib -o mibf_build
//   ./mibf_build refs 31 0.3 a.fa b.fa.gz --seeds 1110111011101110111011101110111,1101101101101101011011011011011
//   ./mibf_build refs 31 0.3 genomes.fa --hashes 3 --per-record --u32
//   ./mibf_classify refs.bf refs.mibf <table size> reads.fq
//
// Writes out_prefix.bf (the stage-1 bit filter, btlbf_store), out_prefix.mibf (the ID array, MIBloomFilter::store) and
// out_prefix.ids.tsv: `id<TAB>path` per file, or with --per-record `id<TAB>path<TAB>record ordinal in that file` per
// record (the parser does not deliver record names).  Prints the report and the table size (largest id + 1) that
// mibf_classify takes as its third argument.  Options: --seeds s1,s2,.. | --hashes N, --u32 (uint32_t ids),
// --per-record, --serial | --no-saturation (default: parallel saturation, one call per batch), --bits N, --entries N,
// --batch-bytes N, --first-id N, --scratch-bytes N (parallel saturation decides a batch at once: the default batch of
// 64 MiB needs 5 GiB of scratch, see btlbf_mibf_build_fastx).
#include "btlbf/MIBloomFilter.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

struct Options {
	std::string prefix;
	std::vector<std::string> paths;
	bool u32 = false;
};

template<typename T>
static int run(const Options& o, const btlbf::MIBFBuildOptions& b)
{
	typedef btlbf::MIBloomFilter<T> MIBF;
	btlbf::MIBFBuildReport rep;
	btlbf_filter* stage1 = nullptr;
	std::unique_ptr<MIBF> miBF(MIBF::buildFromFiles(o.paths, b, &rep, &stage1));
	btlbf_shim::check(btlbf_store(stage1, (o.prefix + ".bf").c_str()));
	btlbf_destroy(stage1);
	miBF->store(o.prefix + ".mibf");
	FILE* tsv = std::fopen((o.prefix + ".ids.tsv").c_str(), "w");
	if (!tsv) {
		std::fprintf(stderr, "error: `%s.ids.tsv' could not be written\n", o.prefix.c_str());
		return 1;
	}
	uint64_t id = b.firstId;
	for (size_t j = 0; j < o.paths.size(); ++j) {
		if (!b.idPerRecord)
			std::fprintf(tsv, "%llu\t%s\n", (unsigned long long)id++, o.paths[j].c_str());
		else
			for (uint64_t r = 0; r < rep.recordsPerFile[j]; ++r)
				std::fprintf(tsv, "%llu\t%s\t%llu\n", (unsigned long long)id++, o.paths[j].c_str(), (unsigned long long)r);
	}
	std::fclose(tsv);
	std::printf("records\t%llu\nids\t%llu\nlongest record\t%llu\nbases\t%llu\nentries\t%llu\nbits\t%llu\npop\t%llu\n",
	            (unsigned long long)rep.n_records, (unsigned long long)rep.n_ids, (unsigned long long)rep.longest_record,
	            (unsigned long long)rep.n_bases, (unsigned long long)rep.entries, (unsigned long long)rep.bits,
	            (unsigned long long)rep.pop);
	std::printf("saturation\tclean %llu\tfound %llu\tmutated %llu\tsaturated %llu\n", (unsigned long long)rep.sat_counts4[0],
	            (unsigned long long)rep.sat_counts4[1], (unsigned long long)rep.sat_counts4[2],
	            (unsigned long long)rep.sat_counts4[3]);
	for (int p = 0; p < 4; ++p)
		std::printf("pass %d\tbatches %llu\tseconds %.6f\tparsing %.6f\n", p, (unsigned long long)rep.batches[p], rep.seconds[p],
		            rep.seconds_parse[p]);
	std::printf("seconds\t%.6f\ntable size\t%llu\n", rep.seconds_total, (unsigned long long)(b.firstId + rep.n_ids));
	return 0;
}

static int usage()
{
	std::fprintf(stderr, "usage: mibf_build <out_prefix> <k> <occupancy> <ref1> [ref2 ...] --seeds s1,s2,.. | --hashes N\n"
	                     "         [--u32] [--per-record] [--serial | --no-saturation] [--bits N] [--entries N]\n"
	                     "         [--batch-bytes N] [--scratch-bytes N] [--first-id N]\n");
	return 2;
}

int main(int argc, char** argv)
{
	Options o;
	btlbf::MIBFBuildOptions b;
	std::vector<std::string> pos;
	for (int i = 1; i < argc; ++i) {
		const std::string a = argv[i];
		auto value = [&]() -> const char* { return i + 1 < argc ? argv[++i] : "0"; };
		if (a == "--u32")
			o.u32 = true;
		else if (a == "--per-record")
			b.idPerRecord = true;
		else if (a == "--serial")
			b.saturation = BTLBF_MIBF_SAT_SERIAL;
		else if (a == "--no-saturation")
			b.saturation = BTLBF_MIBF_SAT_NONE;
		else if (a == "--hashes")
			b.hashNum = (unsigned)std::atoi(value());
		else if (a == "--bits")
			b.bits = std::strtoull(value(), nullptr, 10);
		else if (a == "--entries")
			b.expectedEntries = std::strtoull(value(), nullptr, 10);
		else if (a == "--batch-bytes")
			b.batchBytes = std::strtoull(value(), nullptr, 10);
		else if (a == "--scratch-bytes")
			b.scratchBytes = std::strtoull(value(), nullptr, 10);
		else if (a == "--first-id")
			b.firstId = (uint32_t)std::strtoul(value(), nullptr, 10);
		else if (a == "--seeds") {
			const std::string list = value();
			for (size_t at = 0; at <= list.size();) {
				const size_t comma = std::min(list.find(',', at), list.size());
				b.seeds.push_back(list.substr(at, comma - at));
				at = comma + 1;
			}
		} else if (a.size() > 1 && a[0] == '-' && a[1] == '-')
			return usage();
		else
			pos.push_back(a);
	}
	if (pos.size() < 4 || (b.seeds.empty() == (b.hashNum == 0)))
		return usage();
	o.prefix = pos[0];
	b.kmerSize = (unsigned)std::atoi(pos[1].c_str());
	b.occupancy = std::atof(pos[2].c_str());
	o.paths.assign(pos.begin() + 3, pos.end());
	return o.u32 ? run<uint32_t>(o, b) : run<uint16_t>(o, b);
}
