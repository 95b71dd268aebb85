// tests/cpp/test_card_shim.cpp -- btlbf::KmerCardinality (include/btlbf/KmerCardinality.hpp) over the stub ABI of
// tests/cpp/stub_abi_card.cpp: what the class passes down (buffers, offsets, flags, sizes) and what it hands back, the
// error convention, and that every sketch made is destroyed.  Needs neither the library nor a GPU; built with the
// sanitizers by tests/test_cardinality_solve_cpu.py.
#define BTLBF_SHIM_THROW
#include <btlbf/KmerCardinality.hpp>

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

const std::string& stub_card_log();
int stub_card_live();

static int g_fail = 0;
#define EXPECT(cond)                                                \
	do {                                                            \
		if (!(cond)) {                                              \
			std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
			++g_fail;                                               \
		}                                                           \
	} while (0)

static bool logged(const char* what) { return stub_card_log().find(what) != std::string::npos; }

int main()
{
	{
		btlbf::KmerCardinality card(5, 3, 8, 2);
		EXPECT(logged("create 5 3 8 2") && card.getKmerSize() == 5 && card.sampleBits() == 3 && card.tableBits() == 8);
		EXPECT(stub_card_live() == 1 && card.handle() != nullptr);
		// one sequence; many in one call: the offsets reach the library, an empty read included
		card.add(std::string("ACGTACGT"));
		EXPECT(logged("add_seqs len 8 seqs 1 mem 0 stream 0"));
		card.add(std::vector<std::string>{"ACGTACG", "", "ACGTACGTACGT", "ACG"});
		EXPECT(logged("add_seqs len 22 seqs 4 mem 0 stream 0"));
		card.add(std::vector<std::string>());
		EXPECT(logged("add_seqs len 0 seqs 0 mem 0 stream 0"));
		uint64_t tot[3] = {9, 9, 9};
		std::vector<uint32_t> t = card.table(tot);
		EXPECT(t.size() == 256 && t[8] == 1 && t[7] == 1 && t[0] == 1 && t[12] == 1 && t[3] == 1);
		EXPECT(tot[0] == 4 + 3 + 8 && tot[1] == tot[0] && tot[2] == 5);
		EXPECT(card.table().size() == 256);
		// a raw buffer with a layout, memory space and stream
		const uint64_t starts[3] = {0, 4, 10};
		const btlbf_layout lay = {starts, 2, 0};
		card.add("ACGTACGTAC", 10, &lay, BTLBF_DEVICE, reinterpret_cast<void*>(16));
		EXPECT(logged("add_seqs len 10 seqs 2 mem 1 stream 1"));
		// files: the flag and the batch size
		btlbf_fastx_stats st = card.addFile("reads.fq.gz");
		EXPECT(logged("add_fastx reads.fq.gz") && logged("add_fastx flags 0 batch 0") && st.n_records == 7 && st.n_windows == 70);
		card.addFile("contigs.fa", true, 4096);
		EXPECT(logged("add_fastx contigs.fa") && logged("add_fastx flags 1 batch 4096"));
		// histogram and estimate: every field arrives
		std::vector<uint64_t> h = card.histogram(4);
		EXPECT(h.size() == 4 && h[0] + h[1] + h[2] + h[3] == 256 && h[1] >= 4);
		const btlbf::KmerCardinality::Estimate e = card.estimate(10);
		EXPECT(logged("solve 10 3 8") && e.distinct == 1000.0 + (double)card.histogram(10)[1] && e.singletons == 100.0);
		EXPECT(e.occupancy == 0.25 && e.spectrum.size() == 9 && e.spectrum[0] == 0.0 && e.spectrum[4] == 25.0);
		EXPECT(e.sampled == 7 && e.cleanWindows == e.windows && e.overflowBuckets == 0);
		EXPECT(e.atLeast(1) == e.distinct && e.atLeast(2) == e.distinct - 100.0 && e.atLeast(3) == e.distinct - 150.0);
		EXPECT(card.estimate().spectrum.size() == 63 && logged("solve 64 3 8"));
		const btlbf::KmerCardinality::Estimate s = btlbf::KmerCardinality::solve({250, 4, 2}, 1, 8);
		EXPECT(logged("solve 3 1 8") && s.distinct == 1004.0 && s.overflowBuckets == 2 && s.spectrum.size() == 2 && s.windows == 0);
		// upload, merge, clear
		std::vector<uint32_t> up(256, 0);
		up[200] = 77;
		const uint64_t tot2[3] = {1, 2, 3};
		btlbf::KmerCardinality other(5, 3, 8);
		other.upload(up, tot2);
		card.merge(other);
		t = card.table(tot);
		EXPECT(t[200] == 77 && tot[2] == 7 + 3 && stub_card_live() == 2);
		card.clear();
		EXPECT(logged("clear") && card.table(tot)[200] == 0 && tot[0] == 0);
		// the shims' error convention: an exception under BTLBF_SHIM_THROW, with the library's message
		int thrown = 0;
		try {
			card.addFile("missing.fq");
		} catch (const std::runtime_error& x) {
			thrown += std::string(x.what()).find("could not be read") != std::string::npos;
		}
		try {
			btlbf::KmerCardinality different(5, 3, 9);
			card.merge(different);
		} catch (const std::runtime_error&) {
			++thrown;
		}
		try {
			card.upload(std::vector<uint32_t>(255), tot2);
		} catch (const std::runtime_error&) {
			++thrown;
		}
		try {
			card.histogram(2);
		} catch (const std::runtime_error&) {
			++thrown;
		}
		try {
			btlbf::KmerCardinality bad(5, 3, 40);
		} catch (const std::runtime_error&) {
			++thrown;
		}
		EXPECT(thrown == 5);
	}
	EXPECT(stub_card_live() == 0);
	if (g_fail) {
		std::printf("%d card shim checks failed\n", g_fail);
		return 1;
	}
	std::printf("card shim test passed\n");
	return 0;
}
