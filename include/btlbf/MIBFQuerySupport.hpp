// include/btlbf/MIBFQuerySupport.hpp -- btlbf::MIBFQuerySupport<T>, the reference's read classifier
// (MIBFQuerySupport.hpp) over btlbf_mibf_classify_seqs: same class name, constructor arguments and QueryResult
// (frameProb included).  The reference's query takes a hash iterator and is called once per read; here
//   * query(const std::vector<std::string>& seqs, minCount) classifies a whole batch in one call -- the one to use;
//   * query(const std::string& seq, minCount) is the reference's per-read call and costs ONE GPU ROUND TRIP per read,
//     like the iterator loops of INTEGRATION.md section 1: for porting and small inputs only.
// The paired overload query(itr1, itr2, minCount) (one walk over both mates' frames in turn) is here
//   * queryPairs(seqs1, seqs2, minCount) for a whole batch of pairs in one call (btlbf_mibf_classify_pairs), and
//   * query(seq1, seq2, minCount), the per-pair call, again one GPU round trip each.
// Whole files: queryFile / queryFiles / queryInterleavedFile stream FASTA / FASTQ input through the same classification and
// hand the rows to a callback in file order; summarizeFile returns reads per id only (btlbf_mibf_classify_fastx_*).
// getSatCount() / getEvalCount() answer for the last query(seq) or query(seq1, seq2); the batched queries return them
// per read or pair.  The rules for what the reference leaves open are in include/btlbf.h (btlbf_mibf_classify_seqs).
// Errors follow detail.hpp.
#ifndef BTLBF_MIBFQUERYSUPPORT_HPP
#define BTLBF_MIBFQUERYSUPPORT_HPP
#include "MIBloomFilter.hpp"

#include <cstdint>
#include <string>
#include <vector>

namespace btlbf {

template<typename T>
class MIBFQuerySupport
{
  public:
	// the reference's arguments (MIBFQuerySupport.hpp:33-40); maxResults bounds the records kept per read
	MIBFQuerySupport(const MIBloomFilter<T>& miBF, const std::vector<double>& perFrameProb, double extraCount,
	                 unsigned extraFrameLimit, unsigned maxMiss, unsigned minCount, bool bestHitAgree,
	                 unsigned maxResults = 64)
	  : m_miBF(miBF)
	  , m_perFrameProb(perFrameProb)
	  , m_satCount(0)
	  , m_evalCount(0)
	{
		m_par.extra_count = extraCount;
		m_par.extra_frame_limit = extraFrameLimit;
		m_par.max_miss = maxMiss;
		m_par.min_count = minCount;
		m_par.best_hit_agree = bestHitAgree ? 1 : 0;
		m_par.max_results = maxResults;
	}

	struct QueryResult
	{
		T id;
		uint16_t count;
		uint16_t nonSatCount;
		uint16_t totalCount;
		uint16_t totalNonSatCount;
		uint16_t nonSatFrameCount;
		uint16_t solidCount;
		double frameProb;
	};

	struct BatchResult
	{
		std::vector<std::vector<QueryResult> > results; // per read, at most maxResults each
		std::vector<uint32_t> nResults;                 // per read, all significant results
		std::vector<uint32_t> satCount, evalCount;      // per read
	};

	// one call for all reads
	BatchResult query(const std::vector<std::string>& seqs, const std::vector<unsigned>& minCount) const
	{
		std::string buf;
		std::vector<uint64_t> starts(1, 0);
		for (size_t i = 0; i < seqs.size(); ++i) {
			buf += seqs[i];
			starts.push_back(buf.size());
		}
		return classify(buf, starts, seqs.size(), false, minCount);
	}

	// one call for all pairs: seqs1[i] and seqs2[i] are mate 1 and mate 2 of pair i; one result per pair
	BatchResult queryPairs(const std::vector<std::string>& seqs1, const std::vector<std::string>& seqs2,
	                       const std::vector<unsigned>& minCount) const
	{
		if (seqs1.size() != seqs2.size())
			btlbf_shim::check(BTLBF_EINVAL);
		std::string buf;
		std::vector<uint64_t> starts(1, 0);
		for (size_t i = 0; i < seqs1.size(); ++i) {
			buf += seqs1[i];
			starts.push_back(buf.size());
			buf += seqs2[i];
			starts.push_back(buf.size());
		}
		return classify(buf, starts, seqs1.size(), true, minCount);
	}

	// the reference's per-read call: one GPU round trip
	const std::vector<QueryResult>& query(const std::string& seq, const std::vector<unsigned>& minCount)
	{
		BatchResult b = query(std::vector<std::string>(1, seq), minCount);
		m_signifResults = b.results[0];
		m_satCount = b.satCount[0];
		m_evalCount = b.evalCount[0];
		return m_signifResults;
	}

	// the reference's per-pair call (:111-130): one GPU round trip
	const std::vector<QueryResult>&
	query(const std::string& seq1, const std::string& seq2, const std::vector<unsigned>& minCount)
	{
		BatchResult b = queryPairs(std::vector<std::string>(1, seq1), std::vector<std::string>(1, seq2), minCount);
		m_signifResults = b.results[0];
		m_satCount = b.satCount[0];
		m_evalCount = b.evalCount[0];
		return m_signifResults;
	}

	// The reads of FASTA / FASTQ files (plain or gzip), classified in file order, batch by batch
	// (btlbf_mibf_classify_fastx_*): queryFile -- every record on its own; queryFiles -- record i of path1 and record i
	// of path2 as pair i; queryInterleavedFile -- records 2i and 2i + 1 of one file as pair i.  Per batch
	// sink(firstRow, results, satCounts, evalCounts) is called with the batch's rows (results[r]: at most maxResults
	// records of row firstRow + r; the vectors are the callee's until it returns); a functor passed as an lvalue keeps
	// its state.  Returns the number of rows.
	// batchBytes: bases per batch (0: 64 MiB); a record longer than that is an error.
	template<typename Sink>
	uint64_t queryFile(const std::string& path, const std::vector<unsigned>& minCount, Sink&& sink, uint64_t batchBytes = 0) const
	{
		return classifyFile(path.c_str(), nullptr, 0, minCount, sink, batchBytes);
	}
	template<typename Sink>
	uint64_t queryFiles(const std::string& path1, const std::string& path2, const std::vector<unsigned>& minCount, Sink&& sink,
	                    uint64_t batchBytes = 0) const
	{
		return classifyFile(path1.c_str(), path2.c_str(), 0, minCount, sink, batchBytes);
	}
	template<typename Sink>
	uint64_t queryInterleavedFile(const std::string& path, const std::vector<unsigned>& minCount, Sink&& sink,
	                              uint64_t batchBytes = 0) const
	{
		return classifyFile(path.c_str(), nullptr, BTLBF_CLASSIFY_INTERLEAVED, minCount, sink, batchBytes);
	}

	// reads (or pairs) per id over whole files, no per-read result leaves the GPU (btlbf_mibf_classify_fastx)
	struct FileSummary
	{
		std::vector<uint64_t> best; // per id: rows whose first result is this id
		std::vector<uint64_t> any;  // per id: rows with this id among their first maxResults results
		uint64_t rows, rowsWithoutResult, rowsWithSeveral, rowsTruncated, satCount, evalCount;
	};
	// path2 empty: single reads, or with `interleaved` the pairs of one file
	FileSummary summarizeFile(const std::string& path1, const std::string& path2, const std::vector<unsigned>& minCount,
	                          bool interleaved = false, uint64_t batchBytes = 0) const
	{
		std::vector<uint32_t> mc(minCount.begin(), minCount.end());
		if (mc.size() != m_perFrameProb.size())
			btlbf_shim::check(BTLBF_EINVAL);
		FileSummary out;
		out.best.assign(mc.size() + 1, 0);
		out.any.assign(mc.size() + 1, 0);
		uint64_t t[6] = {0, 0, 0, 0, 0, 0};
		btlbf_shim::check(btlbf_mibf_classify_fastx(m_miBF.handle(), path1.c_str(), path2.empty() ? nullptr : path2.c_str(),
		                                            interleaved ? (uint32_t)BTLBF_CLASSIFY_INTERLEAVED : 0u, &m_par,
		                                            m_perFrameProb.data(), mc.data(), mc.size(), batchBytes, &out.best[0],
		                                            &out.any[0], t, nullptr));
		out.best.resize(mc.size());
		out.any.resize(mc.size());
		out.rows = t[0];
		out.rowsWithoutResult = t[1];
		out.rowsWithSeveral = t[2];
		out.rowsTruncated = t[3];
		out.satCount = t[4];
		out.evalCount = t[5];
		return out;
	}

	unsigned getSatCount() const { return m_satCount; }
	unsigned getEvalCount() const { return m_evalCount; }

  private:
	// the sequences of buf (starts: their offsets) as n rows of single reads or of pairs
	BatchResult classify(const std::string& buf, const std::vector<uint64_t>& starts, size_t n, bool pairs,
	                     const std::vector<unsigned>& minCount) const
	{
		btlbf_layout l;
		l.starts = &starts[0];
		l.n_seqs = starts.size() - 1;
		l.read_len = 0;
		const size_t mr = m_par.max_results;
		std::vector<btlbf_mibf_hit> hits(n * mr + 1);
		BatchResult out;
		out.nResults.assign(n + 1, 0);
		out.satCount.assign(n + 1, 0);
		out.evalCount.assign(n + 1, 0);
		std::vector<uint32_t> mc(minCount.begin(), minCount.end());
		if (mc.size() != m_perFrameProb.size())
			btlbf_shim::check(BTLBF_EINVAL);
		btlbf_shim::check((pairs ? btlbf_mibf_classify_pairs : btlbf_mibf_classify_seqs)(
		    m_miBF.handle(), buf.empty() ? "" : buf.data(), buf.size(), &l, &m_par, m_perFrameProb.data(), mc.data(), mc.size(),
		    &hits[0], &out.nResults[0], &out.satCount[0], &out.evalCount[0], BTLBF_HOST, nullptr));
		out.nResults.resize(n);
		out.satCount.resize(n);
		out.evalCount.resize(n);
		out.results.resize(n);
		for (size_t s = 0; s < n; ++s) {
			const size_t w = out.nResults[s] < mr ? out.nResults[s] : mr;
			for (size_t i = 0; i < w; ++i) {
				const btlbf_mibf_hit& h = hits[s * mr + i];
				QueryResult r = {(T)h.id,           h.count,           h.nonSatCount, h.totalCount,
				                 h.totalNonSatCount, h.nonSatFrameCount, h.solidCount,  m_perFrameProb[h.id]};
				out.results[s].push_back(r);
			}
		}
		return out;
	}

	struct FileHandle // closes on every way out of classifyFile, a throwing sink included
	{
		btlbf_mibf_fastx* c;
		FileHandle() : c(nullptr) {}
		~FileHandle() { btlbf_mibf_classify_fastx_close(c); }
	};

	template<typename Sink>
	uint64_t classifyFile(const char* path1, const char* path2, uint32_t flags, const std::vector<unsigned>& minCount,
	                      Sink& sink, uint64_t batchBytes) const
	{
		std::vector<uint32_t> mc(minCount.begin(), minCount.end());
		if (mc.size() != m_perFrameProb.size())
			btlbf_shim::check(BTLBF_EINVAL);
		FileHandle fh;
		btlbf_shim::check(btlbf_mibf_classify_fastx_open(&fh.c, m_miBF.handle(), path1, path2, flags, &m_par,
		                                                 m_perFrameProb.data(), mc.data(), mc.size(), batchBytes));
		const size_t mr = m_par.max_results;
		uint64_t rows = 0;
		for (;;) {
			uint64_t first = 0, n = 0;
			const btlbf_mibf_hit* hits = nullptr;
			const uint32_t *nHits = nullptr, *sat = nullptr, *ev = nullptr;
			btlbf_shim::check(btlbf_mibf_classify_fastx_next(fh.c, &first, &n, &hits, &nHits, &sat, &ev));
			if (n == 0)
				break;
			std::vector<std::vector<QueryResult> > results(n);
			for (uint64_t s = 0; s < n; ++s) {
				const size_t w = nHits[s] < mr ? nHits[s] : mr;
				for (size_t i = 0; i < w; ++i) {
					const btlbf_mibf_hit& h = hits[s * mr + i];
					QueryResult r = {(T)h.id,           h.count,           h.nonSatCount, h.totalCount,
					                 h.totalNonSatCount, h.nonSatFrameCount, h.solidCount,  m_perFrameProb[h.id]};
					results[s].push_back(r);
				}
			}
			std::vector<uint32_t> satCounts(sat, sat + n), evalCounts(ev, ev + n);
			sink(first, results, satCounts, evalCounts);
			rows += n;
		}
		return rows;
	}

	const MIBloomFilter<T>& m_miBF;
	const std::vector<double> m_perFrameProb;
	btlbf_mibf_classify_params m_par;
	unsigned m_satCount, m_evalCount;
	std::vector<QueryResult> m_signifResults;
};

} // namespace btlbf
#endif
