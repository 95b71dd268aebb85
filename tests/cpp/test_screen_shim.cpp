// tests/cpp/test_screen_shim.cpp -- btlbf::ReadScreen (include/btlbf/ReadScreen.hpp) for tests/test_gpu_cpp_screen.py:
// loads two stored filters, screens the reads of a FASTQ file three ways -- screen() on the sequence lines it reads
// itself, screenFile() through a functor, summarizeFile() -- and dumps every row and total, so that the Python side can
// compare all of it.
// argv: a.bf b.bf reads.fq min_fraction min_hits batch_bytes
#define BTLBF_SHIM_THROW
#include <btlbf/ReadScreen.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

struct Rows {
	uint64_t rows = 0, next = 0, batches = 0;
	bool contiguous = true;
	const char* tag;
	explicit Rows(const char* t) : tag(t) {}
	void operator()(uint64_t first, const btlbf::ReadScreen::Result& r)
	{
		contiguous = contiguous && first == next && r.hits.size() == r.rows() * r.nFilters && r.passBits.size() == r.rows();
		next = first + r.rows();
		rows += r.rows();
		++batches;
		for (size_t i = 0; i < r.rows(); ++i) {
			std::printf("%s %llu", tag, (unsigned long long)(first + i));
			for (size_t j = 0; j < r.nFilters; ++j)
				std::printf(" %u", r.hit(i, j));
			std::printf(" %u %u\n", r.valid[i], r.passBits[i]);
		}
	}
};

int main(int argc, char** argv)
{
	if (argc != 7)
		return 2;
	try {
		BloomFilter a(argv[1]), b(argv[2]);
		const btlbf::ReadScreen screen({&a, &b}, std::atof(argv[4]), (unsigned)std::atoi(argv[5]));
		const uint64_t batchBytes = std::strtoull(argv[6], nullptr, 10);
		std::vector<std::string> reads;
		std::ifstream in(argv[3]);
		std::string line;
		for (size_t i = 0; std::getline(in, line); ++i)
			if (i % 4 == 1)
				reads.push_back(line);
		Rows mem("mem");
		mem(0, screen.screen(reads));
		Rows file("file");
		const uint64_t n = screen.screenFile(argv[3], file, batchBytes);
		std::printf("file_rows %llu %llu %d\n", (unsigned long long)n, (unsigned long long)file.batches,
		            (int)(file.contiguous && file.rows == n));
		const btlbf::ReadScreen::FileSummary s = screen.summarizeFile(argv[3], batchBytes);
		std::printf("passed %llu %llu\nbest %llu %llu\n", (unsigned long long)s.passed[0], (unsigned long long)s.passed[1],
		            (unsigned long long)s.best[0], (unsigned long long)s.best[1]);
		std::printf("totals %llu %llu %llu %llu\n", (unsigned long long)s.rows, (unsigned long long)s.rowsPassingNone,
		            (unsigned long long)s.rowsPassingSeveral, (unsigned long long)s.rowsWithoutKmer);
		std::printf("stats %llu %llu %llu\n", (unsigned long long)s.stats.n_records, (unsigned long long)s.stats.n_bases,
		            (unsigned long long)s.stats.n_windows);
		// the shims' error convention: an exception under BTLBF_SHIM_THROW
		try {
			const btlbf::ReadScreen twice({&a, &a});
			twice.screen(reads);
			std::printf("refused 0\n");
		} catch (const std::runtime_error& e) {
			std::printf("refused 1 %s\n", e.what());
		}
	} catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	return 0;
}
