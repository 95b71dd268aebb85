// include/btlbf/KmerCardinality.hpp -- how many distinct k-mers do these reads hold, and how many of them occur once,
// twice, ...: the numbers a filter is sized from (btlbf_card_* of btlbf.h).
//
// The reference's constructors take them as given -- BloomFilter(expectedElemNum, fpr, hashNum, kmerSize),
// MIBloomFilter<T>::calcOptimalSize(entries, ...) -- and its users get them from a streaming estimator before they build
// anything.  KmerCardinality is that estimator for this library: a sampled, bucketed sketch of the reads' canonical
// ntHash values, built in HBM in one pass and solved on the host.  Errors follow the shims' convention (detail.hpp):
// exit(1), or exceptions under BTLBF_SHIM_THROW.
//
//   btlbf::KmerCardinality card(31);
//   card.addFile("reads.fq.gz");
//   auto e = card.estimate();                              // e.distinct, e.singletons, e.spectrum[i] = f_i, e.occupancy
//   BloomFilter all(size_t(e.distinct), 0.01, 0, 31);      // every k-mer
//   size_t solid = size_t(e.atLeast(3));                   // ... or those seen three times and more
#ifndef BTLBF_KMERCARDINALITY_HPP
#define BTLBF_KMERCARDINALITY_HPP
#include "detail.hpp"

#include <string>
#include <vector>

namespace btlbf {

class KmerCardinality
{
  public:
	static const unsigned kDefaultSampleBits = 11, kDefaultTableBits = 22;

	struct Estimate
	{
		double distinct;   // F0: the distinct k-mers
		double singletons; // f1: those seen once
		double occupancy;  // the share of the sketch's counters in use: trust the estimate between about 0.05 and 0.8
		uint64_t windows, cleanWindows, sampled;
		uint64_t overflowBuckets;
		std::vector<double> spectrum; // spectrum[i] = f_i, the distinct k-mers seen i times; spectrum[0] = 0
		// the distinct k-mers seen at least T times (T >= 1): distinct - (f_1 + ... + f_{T-1})
		double atLeast(unsigned T) const
		{
			double below = 0;
			for (size_t i = 1; i < T && i < spectrum.size(); ++i)
				below += spectrum[i];
			return distinct - below;
		}
	};

	// a window is sampled when the top sampleBits bits of its mixed hash are zero; 2^tableBits 32-bit counters in HBM
	explicit KmerCardinality(unsigned kmerSize, unsigned sampleBits = kDefaultSampleBits, unsigned tableBits = kDefaultTableBits,
	                         int device = btlbf_shim::default_device())
	  : m_c(nullptr), m_k(kmerSize), m_s(sampleBits), m_r(tableBits)
	{
		btlbf_shim::check(btlbf_card_create(&m_c, kmerSize, sampleBits, tableBits, device));
	}
	~KmerCardinality() { btlbf_card_destroy(m_c); }
	KmerCardinality(const KmerCardinality&) = delete;
	KmerCardinality& operator=(const KmerCardinality&) = delete;

	unsigned getKmerSize() const { return m_k; }
	unsigned sampleBits() const { return m_s; }
	unsigned tableBits() const { return m_r; }
	btlbf_card* handle() const { return m_c; }

	void clear() { btlbf_shim::check(btlbf_card_clear(m_c)); }

	// the k-mers of one sequence, or of many in one GPU round trip; calls accumulate
	void add(const std::string& seq)
	{
		btlbf_shim::check(btlbf_card_add_seqs(m_c, seq.data(), seq.size(), nullptr, BTLBF_HOST, nullptr));
	}
	void add(const std::vector<std::string>& reads)
	{
		std::string buf;
		std::vector<uint64_t> starts(1, 0);
		for (size_t i = 0; i < reads.size(); ++i) {
			buf += reads[i];
			starts.push_back(buf.size());
		}
		btlbf_layout l;
		l.starts = &starts[0];
		l.n_seqs = reads.size();
		l.read_len = 0;
		btlbf_shim::check(btlbf_card_add_seqs(m_c, buf.empty() ? "" : buf.data(), buf.size(), &l, BTLBF_HOST, nullptr));
	}
	// a buffer in the library's layouts, in host or device memory (btlbf_card_add_seqs)
	void add(const char* seq, uint64_t len, const btlbf_layout* layout, int mem = BTLBF_HOST, void* stream = nullptr)
	{
		btlbf_shim::check(btlbf_card_add_seqs(m_c, seq, len, layout, mem, stream));
	}
	// the records of a FASTA / FASTQ file, plain or gzip (perLine: every sequence line is a sequence of its own)
	btlbf_fastx_stats addFile(const std::string& path, bool perLine = false, uint64_t batchBytes = 0)
	{
		btlbf_fastx_stats st;
		btlbf_shim::check(btlbf_card_add_fastx(m_c, path.c_str(), perLine ? BTLBF_FASTX_LINES : 0, batchBytes, &st));
		return st;
	}
	// the sketch of this input and the other's (same k-mer size, sampleBits, tableBits and device)
	void merge(const KmerCardinality& other) { btlbf_shim::check(btlbf_card_merge(m_c, other.m_c)); }

	std::vector<uint32_t> table(uint64_t totals3[3] = nullptr) const
	{
		std::vector<uint32_t> t(size_t(1) << m_r);
		uint64_t tot[3];
		btlbf_shim::check(btlbf_card_download(m_c, &t[0], tot));
		for (int i = 0; totals3 && i < 3; ++i)
			totals3[i] = tot[i];
		return t;
	}
	void upload(const std::vector<uint32_t>& table, const uint64_t totals3[3])
	{
		if (table.size() != size_t(1) << m_r || !totals3)
			btlbf_shim::check(BTLBF_EINVAL);
		btlbf_shim::check(btlbf_card_upload(m_c, &table[0], totals3));
	}
	// t[i] = counters equal to i, the last entry those at or above nHist - 1
	std::vector<uint64_t> histogram(unsigned nHist) const
	{
		std::vector<uint64_t> t(nHist ? nHist : 1);
		btlbf_shim::check(btlbf_card_histogram(m_c, &t[0], nHist));
		return t;
	}
	// the spectrum up to f_{nHist-2}
	Estimate estimate(unsigned nHist = 64) const
	{
		btlbf_card_estimate e;
		std::vector<double> f(nHist > 1 ? nHist - 1 : 1);
		btlbf_shim::check(btlbf_card_estimate_now(m_c, nHist, &e, &f[0]));
		return make(e, f);
	}
	// ... from a histogram alone: host arithmetic, no GPU
	static Estimate solve(const std::vector<uint64_t>& t, unsigned sampleBits, unsigned tableBits)
	{
		btlbf_card_estimate e;
		std::vector<double> f(t.size() > 1 ? t.size() - 1 : 1);
		btlbf_shim::check(btlbf_card_solve(t.empty() ? nullptr : &t[0], (unsigned)t.size(), sampleBits, tableBits, &e, &f[0]));
		return make(e, f);
	}

  private:
	static Estimate make(const btlbf_card_estimate& e, const std::vector<double>& f)
	{
		Estimate out;
		out.distinct = e.distinct;
		out.singletons = e.singletons;
		out.occupancy = e.occupancy;
		out.windows = e.windows;
		out.cleanWindows = e.clean_windows;
		out.sampled = e.sampled;
		out.overflowBuckets = e.overflow_buckets;
		out.spectrum = f;
		return out;
	}

	btlbf_card* m_c;
	unsigned m_k, m_s, m_r;
};

} // namespace btlbf
#endif
