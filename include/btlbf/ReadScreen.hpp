// include/btlbf/ReadScreen.hpp -- reads against several Bloom filters in one pass (btlbf_screen_* of btlbf.h).
//
// The reference has no such class: a caller screens reads by looping over filters and k-mers,
//   for each filter: ntHashIterator itr(seq, h, k); while (itr != itr.end()) { hits += bloom.contains(*itr); ++itr; }
// (BloomFilter.hpp:247-262), and keeps hits / k-mers per read and filter.  ReadScreen does that loop for a batch of reads
// and up to BTLBF_SCREEN_MAX_FILTERS filters of one k-mer size, hash count and seed set in one GPU pass that hashes every
// k-mer once.  Errors follow the shims' convention (detail.hpp): exit(1), or exceptions under BTLBF_SHIM_THROW.
//
//   btlbf::ReadScreen screen({&genome, &contaminants}, 0.5);
//   auto r = screen.screen(reads);            // r.hits[read][filter], r.valid[read], r.passBits[read]
//   screen.screenFile("reads.fq.gz", sink);   // sink(firstRow, const Result&) per batch, in file order
//   auto s = screen.summarizeFile("reads.fq.gz");
#ifndef BTLBF_READSCREEN_HPP
#define BTLBF_READSCREEN_HPP
#include "BloomFilter.hpp"

#include <string>
#include <vector>

namespace btlbf {

class ReadScreen
{
  public:
	// rows of one call or batch
	struct Result
	{
		size_t nFilters;
		std::vector<uint32_t> hits;     // [row * nFilters + filter]: clean k-mers of the read found in the filter
		std::vector<uint32_t> valid;    // [row]: clean k-mers of the read
		std::vector<uint32_t> passBits; // [row]: bit j = the read passes filter j
		size_t rows() const { return valid.size(); }
		uint32_t hit(size_t row, size_t filter) const { return hits[row * nFilters + filter]; }
		bool passes(size_t row, size_t filter) const { return (passBits[row] >> filter) & 1u; }
	};
	struct FileSummary
	{
		std::vector<uint64_t> passed; // per filter: reads passing it
		std::vector<uint64_t> best;   // per filter: reads whose passing filter with the most hits it is (ties: the first)
		uint64_t rows, rowsPassingNone, rowsPassingSeveral, rowsWithoutKmer;
		btlbf_fastx_stats stats;
	};

	// a read passes a filter when it has k-mers, at least minHits of them are in the filter, and at least minFraction
	explicit ReadScreen(const std::vector<BloomFilter*>& filters, double minFraction = 0.0, unsigned minHits = 1)
	{
		for (size_t i = 0; i < filters.size(); ++i)
			m_filters.push_back(filters[i] ? filters[i]->handle() : nullptr);
		m_par.min_fraction = minFraction;
		m_par.min_hits = minHits;
		m_par.reserved = 0;
	}

	size_t size() const { return m_filters.size(); }

	// every read of `reads` against every filter: one GPU round trip
	Result screen(const std::vector<std::string>& reads) const
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
		const size_t n = reads.size(), nf = m_filters.size();
		Result out;
		out.nFilters = nf;
		out.hits.assign(n * nf + 1, 0);
		out.valid.assign(n + 1, 0);
		out.passBits.assign(n + 1, 0);
		btlbf_shim::check(btlbf_screen_seqs(handles(), (unsigned)nf, buf.empty() ? "" : buf.data(), buf.size(), &l, &m_par,
		                                    &out.hits[0], &out.valid[0], &out.passBits[0], BTLBF_HOST, nullptr));
		out.hits.resize(n * nf);
		out.valid.resize(n);
		out.passBits.resize(n);
		return out;
	}

	// The records of a FASTA / FASTQ file (plain or gzip) in file order, batch by batch (btlbf_screen_fastx_*):
	// sink(firstRow, result) per batch (the result is the callee's until it returns; a functor passed as an lvalue keeps
	// its state).  Returns the number of rows.  batchBytes: bases per batch (0: 64 MiB); a longer record is an error.
	template<typename Sink>
	uint64_t screenFile(const std::string& path, Sink&& sink, uint64_t batchBytes = 0) const
	{
		FileHandle fh;
		btlbf_shim::check(btlbf_screen_fastx_open(&fh.c, handles(), (unsigned)m_filters.size(), path.c_str(), 0, &m_par, batchBytes));
		const size_t nf = m_filters.size();
		uint64_t rows = 0;
		for (;;) {
			uint64_t first = 0, n = 0;
			const uint32_t *hits = nullptr, *valid = nullptr, *pass = nullptr;
			btlbf_shim::check(btlbf_screen_fastx_next(fh.c, &first, &n, &hits, &valid, &pass));
			if (n == 0)
				break;
			Result r;
			r.nFilters = nf;
			r.hits.assign(hits, hits + n * nf);
			r.valid.assign(valid, valid + n);
			r.passBits.assign(pass, pass + n);
			sink(first, r);
			rows += n;
		}
		return rows;
	}

	// reads per filter over a whole file; no per-read result leaves the GPU (btlbf_screen_fastx)
	FileSummary summarizeFile(const std::string& path, uint64_t batchBytes = 0) const
	{
		const size_t nf = m_filters.size();
		FileSummary out;
		out.passed.assign(nf + 1, 0);
		out.best.assign(nf + 1, 0);
		uint64_t t[4] = {0, 0, 0, 0};
		btlbf_shim::check(btlbf_screen_fastx(handles(), (unsigned)nf, path.c_str(), 0, &m_par, batchBytes, &out.passed[0],
		                                     &out.best[0], t, &out.stats));
		out.passed.resize(nf);
		out.best.resize(nf);
		out.rows = t[0];
		out.rowsPassingNone = t[1];
		out.rowsPassingSeveral = t[2];
		out.rowsWithoutKmer = t[3];
		return out;
	}

  private:
	struct FileHandle // closes on every way out of screenFile, a throwing sink included
	{
		btlbf_screen_file* c;
		FileHandle() : c(nullptr) {}
		~FileHandle() { btlbf_screen_fastx_close(c); }
	};
	btlbf_filter* const* handles() const { return m_filters.empty() ? nullptr : &m_filters[0]; }

	std::vector<btlbf_filter*> m_filters;
	btlbf_screen_params m_par;
};

} // namespace btlbf
#endif
