// The parser's BTLBF_FASTX_WHOLE mode (csrc/fastx.cpp) as a stand-alone program, for AddressSanitizer and
// UndefinedBehaviorSanitizer on the host code (tests/test_fastx_whole_asan_cpu.py builds fastx.cpp and this file with
// -fsanitize=address,undefined and runs the result; nothing is loaded into Python).  Random FASTQ files -- empty reads,
// CRLF line ends, reads as long as a batch -- at every batch size from the longest read up: the sequences delivered must
// be the records, whole, in order; one byte less than the longest read must fail with EINVAL.  Then a gzipped FASTQ cut
// in half and one with a byte flipped in the middle: BTLBF_EIO from the call that meets the damage and from every later
// one, whole reads of the original before it, and the record count kept.  No GPU: the buffers are pageable.
#include "../../include/btlbf.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include <zlib.h>

// the library's error plumbing (capi.cpp), which this program does not link
static char g_err[512];
int btlbf_set_error(int code, const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	return code;
}
extern "C" const char* btlbf_last_error(void) { return g_err; }
// run_fastx (the bit filter's file path, not exercised here) refers to these
extern "C" unsigned btlbf_kmer_size(const btlbf_filter*) { return 0; }
extern "C" uint64_t btlbf_local_bytes(const btlbf_filter*) { return 0; }
extern "C" int btlbf_device(const btlbf_filter*) { return 0; }
extern "C" int btlbf_contains_seqs(btlbf_filter*, const char*, uint64_t, const btlbf_layout*, uint64_t*, uint64_t*, uint64_t*,
                                   int, void*)
{
	return BTLBF_EHIP;
}
extern "C" int btlbf_insert_seqs(btlbf_filter*, const char*, uint64_t, const btlbf_layout*, int, int, int, void*)
{
	return BTLBF_EHIP;
}

#define CHECK(c)                                                                 \
	do {                                                                         \
		if (!(c)) {                                                              \
			std::printf("FAILED %s (line %d, case %d)\n", #c, __LINE__, g_case); \
			return 1;                                                            \
		}                                                                        \
	} while (0)
static int g_case = 0;

// a damaged .gz: every sequence delivered before the error is the next read of the original, whole (BTLBF_FASTX_WHOLE),
// or a piece of it (without); the error is BTLBF_EIO, names the file, and stays
static int damaged(const std::string& path, const std::vector<std::string>& reads, uint32_t flags, uint64_t batch,
                   bool expect_some)
{
	btlbf_fastx* r = nullptr;
	CHECK(btlbf_fastx_open(&r, path.c_str(), flags | BTLBF_FASTX_PAGEABLE, 31, batch) == BTLBF_OK);
	size_t at = 0, seqs = 0;
	int rc;
	for (;;) {
		const char* bases;
		const uint64_t* starts;
		uint64_t nb, ns;
		rc = btlbf_fastx_next(r, &bases, &nb, &starts, &ns);
		if (rc) {
			CHECK(ns == 0 && nb == 0);
			break;
		}
		CHECK(ns != 0); // a damaged file has no regular end
		for (uint64_t s = 0; s < ns; ++s, ++seqs) {
			const std::string got(bases + starts[s], starts[s + 1] - starts[s]);
			if (flags & BTLBF_FASTX_WHOLE) {
				CHECK(at < reads.size() && got == reads[at]);
				++at;
			} else {
				// a piece of the read at `at` or of the one after it (which of the two: the Python test follows the cuts)
				CHECK(at < reads.size());
				if (reads[at].find(got) == std::string::npos) {
					++at;
					CHECK(at < reads.size() && reads[at].find(got) != std::string::npos);
				}
			}
		}
	}
	CHECK(rc == BTLBF_EIO && std::string(g_err).find(path) != std::string::npos);
	std::printf("%s flags %u batch %llu: %zu sequences, %llu records before \"%s\"\n", path.c_str(), flags,
	            (unsigned long long)batch, seqs, (unsigned long long)btlbf_fastx_records(r), g_err);
	CHECK(at < reads.size());
	if (expect_some)
		CHECK(seqs > reads.size() / 4 && btlbf_fastx_records(r) >= seqs / 2);
	const char* bases;
	const uint64_t* starts;
	uint64_t nb, ns;
	const uint64_t records = btlbf_fastx_records(r);
	CHECK(btlbf_fastx_next(r, &bases, &nb, &starts, &ns) == BTLBF_EIO && ns == 0); // and again
	CHECK(btlbf_fastx_records(r) == records);
	btlbf_fastx_close(r);
	return 0;
}

static int damaged_files(const std::string& path)
{
	std::mt19937_64 rng(11);
	std::vector<std::string> reads(3000);
	const std::string good = path + ".good.gz", cut = path + ".cut.gz", flipped = path + ".flipped.gz";
	gzFile z = gzopen(good.c_str(), "wb");
	CHECK(z);
	for (size_t i = 0; i < reads.size(); ++i) {
		const size_t len = 60 + rng() % 91;
		std::string qual;
		for (size_t j = 0; j < len; ++j) {
			reads[i] += "ACGTN"[rng() % 5];
			qual += "@>+IJ#"[rng() % 6];
		}
		CHECK(gzprintf(z, "@r%zu\n%s\n+\n%s\n", i, reads[i].c_str(), qual.c_str()) > 0);
	}
	CHECK(gzclose(z) == Z_OK);
	std::vector<char> data;
	FILE* f = fopen(good.c_str(), "rb");
	CHECK(f);
	for (int c; (c = fgetc(f)) != EOF;)
		data.push_back((char)c);
	fclose(f);
	CHECK(data.size() > 100000);
	f = fopen(cut.c_str(), "wb");
	CHECK(f && fwrite(data.data(), 1, data.size() / 2, f) == data.size() / 2);
	fclose(f);
	data[data.size() / 2] ^= (char)0xFF;
	f = fopen(flipped.c_str(), "wb");
	CHECK(f && fwrite(data.data(), 1, data.size(), f) == data.size());
	fclose(f);
	for (uint32_t flags : {0u, (uint32_t)BTLBF_FASTX_WHOLE})
		for (uint64_t batch : {(uint64_t)0, (uint64_t)4096}) {
			if (damaged(cut, reads, flags, batch, batch != 0) || damaged(flipped, reads, flags, batch, false))
				return 1;
		}
	return 0;
}

int main(int argc, char** argv)
{
	if (argc != 2)
		return 2;
	const std::string path = argv[1];
	std::mt19937_64 rng(7);
	for (g_case = 0; g_case < 300; ++g_case) {
		const bool crlf = g_case % 3 == 1;
		const size_t n = 1 + rng() % 40, max_len = 1 + rng() % 200;
		std::vector<std::string> reads(n);
		size_t longest = 0;
		FILE* f = fopen(path.c_str(), "wb");
		CHECK(f);
		for (size_t i = 0; i < n; ++i) {
			const size_t len = rng() % 5 == 0 ? 0 : rng() % 7 == 0 ? max_len : rng() % (max_len + 1);
			for (size_t j = 0; j < len; ++j)
				reads[i] += "ACGTN"[rng() % 5];
			longest = reads[i].size() > longest ? reads[i].size() : longest;
			const char* nl = crlf ? "\r\n" : "\n";
			fprintf(f, "@r%zu%s%s%s+%s%s%s", i, nl, reads[i].c_str(), nl, nl, std::string(reads[i].size(), 'I').c_str(), nl);
		}
		fclose(f);
		if (longest == 0)
			longest = 1;
		for (uint64_t batch : {(uint64_t)longest, (uint64_t)longest + 1, (uint64_t)longest * 2 + 3, (uint64_t)1 << 16}) {
			btlbf_fastx* r = nullptr;
			CHECK(btlbf_fastx_open(&r, path.c_str(), BTLBF_FASTX_WHOLE | BTLBF_FASTX_PAGEABLE, 31, batch) == BTLBF_OK);
			size_t at = 0;
			for (;;) {
				const char* bases;
				const uint64_t* starts;
				uint64_t nb, ns;
				CHECK(btlbf_fastx_next(r, &bases, &nb, &starts, &ns) == BTLBF_OK);
				if (ns == 0)
					break;
				CHECK(starts[0] == 0 && starts[ns] == nb && nb <= batch);
				for (uint64_t s = 0; s < ns; ++s, ++at) {
					CHECK(at < n && starts[s] <= starts[s + 1]);
					CHECK(std::string(bases + starts[s], starts[s + 1] - starts[s]) == reads[at]);
				}
			}
			CHECK(at == n && btlbf_fastx_records(r) == n);
			btlbf_fastx_close(r);
		}
		if (longest > 1) {
			btlbf_fastx* r = nullptr;
			CHECK(btlbf_fastx_open(&r, path.c_str(), BTLBF_FASTX_WHOLE | BTLBF_FASTX_PAGEABLE, 31, longest - 1) == BTLBF_OK);
			int rc = BTLBF_OK;
			for (;;) {
				const char* bases;
				const uint64_t* starts;
				uint64_t nb, ns = 0;
				rc = btlbf_fastx_next(r, &bases, &nb, &starts, &ns);
				if (rc || ns == 0)
					break;
			}
			CHECK(rc == BTLBF_EINVAL && std::string(g_err).find("record ") != std::string::npos);
			btlbf_fastx_close(r);
		}
	}
	g_case = -1;
	if (damaged_files(path))
		return 1;
	std::printf("fastx whole test passed\n");
	return 0;
}
