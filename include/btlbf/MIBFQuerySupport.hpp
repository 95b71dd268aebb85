// include/btlbf/MIBFQuerySupport.hpp -- btlbf::MIBFQuerySupport<T>, the reference's read classifier
// (MIBFQuerySupport.hpp) over btlbf_mibf_classify_seqs: same class name, constructor arguments and QueryResult
// (frameProb included).  The reference's query takes a hash iterator and is called once per read; here
//   * query(const std::vector<std::string>& seqs, minCount) classifies a whole batch in one call -- the one to use;
//   * query(const std::string& seq, minCount) is the reference's per-read call and costs ONE GPU ROUND TRIP per read,
//     like the iterator loops of INTEGRATION.md section 1: for porting and small inputs only.
// getSatCount() / getEvalCount() answer for the last query(seq); the batched query returns them per read.
// The rules for what the reference leaves open are in include/btlbf.h (btlbf_mibf_classify_seqs).  The paired overload
// query(itr1, itr2, minCount) is not provided.  Errors follow detail.hpp.
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
		btlbf_layout l;
		l.starts = &starts[0];
		l.n_seqs = seqs.size();
		l.read_len = 0;
		const size_t n = seqs.size(), mr = m_par.max_results;
		std::vector<btlbf_mibf_hit> hits(n * mr + 1);
		BatchResult out;
		out.nResults.assign(n + 1, 0);
		out.satCount.assign(n + 1, 0);
		out.evalCount.assign(n + 1, 0);
		std::vector<uint32_t> mc(minCount.begin(), minCount.end());
		if (mc.size() != m_perFrameProb.size())
			btlbf_shim::check(BTLBF_EINVAL);
		btlbf_shim::check(btlbf_mibf_classify_seqs(m_miBF.handle(), buf.empty() ? "" : buf.data(), buf.size(), &l, &m_par,
		                                           m_perFrameProb.data(), mc.data(), mc.size(), &hits[0], &out.nResults[0],
		                                           &out.satCount[0], &out.evalCount[0], BTLBF_HOST, nullptr));
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

	// the reference's per-read call: one GPU round trip
	const std::vector<QueryResult>& query(const std::string& seq, const std::vector<unsigned>& minCount)
	{
		BatchResult b = query(std::vector<std::string>(1, seq), minCount);
		m_signifResults = b.results[0];
		m_satCount = b.satCount[0];
		m_evalCount = b.evalCount[0];
		return m_signifResults;
	}

	unsigned getSatCount() const { return m_satCount; }
	unsigned getEvalCount() const { return m_evalCount; }

  private:
	const MIBloomFilter<T>& m_miBF;
	const std::vector<double> m_perFrameProb;
	btlbf_mibf_classify_params m_par;
	unsigned m_satCount, m_evalCount;
	std::vector<QueryResult> m_signifResults;
};

} // namespace btlbf
#endif
