// include/btlbf/MIBloomFilter.hpp -- btlbf::MIBloomFilter<T>, the reference's multi-index Bloom filter
// (MIBloomFilter.hpp, MIBFConstructSupport.hpp) over the C ABI's btlbf_mibf_* block: the ID array
// lives in MI355X HBM and every call forwards to the HIP kernels.  T is uint16_t or uint32_t.
//   * construction: from a stage-1 bit filter (MIBloomFilter(hashNum, k, bv, seeds), :122-147) or from a data file
//     plus that filter (MIBloomFilter(path), :149-248; the bit vector is not read from a .sdsl file).
//   * calcFrameProbs / calcProbSingleFrame as in the reference (the perFrameProb table of MIBFQuerySupport).
//   * buildFromFiles: stages 1-4 from FASTA / FASTQ files in one call (btlbf_mibf_build_fastx), what a caller of
//     MIBFConstructSupport writes by hand; calcOptimalSize with the reference's name and arithmetic.
//   * batch members instead of per-k-mer iterators: insertIDs (insertMIBF), insertSaturation, query
//     (getMatchSignature) over sequence buffers with a layout and one id per sequence.
// Errors follow detail.hpp (message + exit(1), or std::runtime_error with BTLBF_SHIM_THROW).
#ifndef BTLBF_MIBLOOMFILTER_HPP
#define BTLBF_MIBLOOMFILTER_HPP
#include "detail.hpp"

#include <cstdint>
#include <string>
#include <vector>

namespace btlbf {

// buildFromFiles' arguments: btlbf_mibf_build_params with the seeds as strings (empty: plain ntHash with hashNum
// values; otherwise one value per seed) and the id width taken from T
// (MIBloomFilter<T>::BuildOptions / ::BuildReport for every T)
struct MIBFBuildOptions
{
	unsigned kmerSize = 0, hashNum = 0;
	std::vector<std::string> seeds;
	uint64_t bits = 0, expectedEntries = 0;
	double occupancy = 0.5;
	bool idPerRecord = false;
	uint32_t firstId = 1;
	int saturation = BTLBF_MIBF_SAT_PARALLEL;
	bool perLine = false;
	uint64_t batchBytes = 0, scratchBytes = 0;
	int device = 0;
};
struct MIBFBuildReport : btlbf_mibf_build_report
{
	std::vector<uint64_t> recordsPerFile;
};

template<typename T>
class MIBloomFilter
{
  public:
	static const T s_mask = (T)((T)1 << (sizeof(T) * 8 - 1));
	static const T s_antiMask = (T)~s_mask;

	// from a stage-1 bit filter (spaced seeds, if any, with h2 = 1); the filter may be destroyed afterwards
	explicit MIBloomFilter(btlbf_filter* stage1) { btlbf_shim::check(btlbf_mibf_create(&m_m, stage1, sizeof(T))); }

	// a data file of store() plus the stage-1 bit filter it was built on
	MIBloomFilter(const std::string& filterFilePath, btlbf_filter* stage1)
	{
		btlbf_shim::check(btlbf_mibf_load(&m_m, filterFilePath.c_str(), stage1, sizeof(T)));
	}

	typedef MIBFBuildOptions BuildOptions;
	typedef MIBFBuildReport BuildReport;

	// calcOptimalSize (MIBloomFilter.hpp:84-88)
	static size_t calcOptimalSize(size_t entries, unsigned hashNum, double occupancy)
	{
		return btlbf_mibf_optimal_size(entries, hashNum, occupancy);
	}

	// stages 1-4 over the files, in order (the contract is btlbf_mibf_build_fastx's); the caller owns the result and,
	// when asked for, the stage-1 filter (store it with btlbf_store: the data file of store() does not hold the bits)
	static MIBloomFilter<T>* buildFromFiles(const std::vector<std::string>& paths, const BuildOptions& o,
	                                        BuildReport* report = nullptr, btlbf_filter** stage1 = nullptr)
	{
		std::vector<const char*> pp, sp;
		for (size_t i = 0; i < paths.size(); ++i)
			pp.push_back(paths[i].c_str());
		for (size_t i = 0; i < o.seeds.size(); ++i)
			sp.push_back(o.seeds[i].c_str());
		btlbf_mibf_build_params p;
		p.kmer_size = o.kmerSize;
		p.hash_num = o.seeds.empty() ? o.hashNum : (unsigned)o.seeds.size();
		p.seeds = sp.empty() ? nullptr : &sp[0];
		p.n_seeds = (unsigned)sp.size();
		p.id_bytes = sizeof(T);
		p.bits = o.bits;
		p.expected_entries = o.expectedEntries;
		p.occupancy = o.occupancy;
		p.id_mode = o.idPerRecord ? BTLBF_MIBF_ID_PER_RECORD : BTLBF_MIBF_ID_PER_FILE;
		p.first_id = o.firstId;
		p.saturation = o.saturation;
		p.fastx_flags = o.perLine ? BTLBF_FASTX_LINES : 0;
		p.batch_bytes = o.batchBytes;
		p.scratch_bytes = o.scratchBytes;
		p.device = o.device;
		std::vector<uint64_t> perFile(paths.size() + 1, 0);
		btlbf_mibf* m = nullptr;
		btlbf_shim::check(btlbf_mibf_build_fastx(&m, stage1, pp.empty() ? nullptr : &pp[0], (unsigned)pp.size(), &p, report,
		                                         &perFile[0]));
		if (report)
			report->recordsPerFile.assign(perFile.begin(), perFile.begin() + paths.size());
		return new MIBloomFilter<T>(m);
	}

	~MIBloomFilter() { btlbf_mibf_destroy(m_m); }
	MIBloomFilter(const MIBloomFilter&) = delete;
	MIBloomFilter& operator=(const MIBloomFilter&) = delete;

	size_t getPop() const { return btlbf_mibf_size(m_m); }
	size_t size() const { return btlbf_mibf_bits(m_m); }
	unsigned getHashNum() const { return btlbf_mibf_hash_num(m_m); }
	unsigned getKmerSize() const { return btlbf_mibf_kmer_size(m_m); }

	size_t getPopNonZero() const { return stats()[1]; }
	size_t getPopSaturated() const { return stats()[2]; }

	// getIDCounts (MIBloomFilter.hpp:539-551): counts[id] += entries per id; returns the saturated entries
	size_t getIDCounts(std::vector<size_t>& counts) const
	{
		std::vector<uint64_t> c(counts.size(), 0);
		uint64_t sat = 0;
		btlbf_shim::check(btlbf_mibf_id_counts(m_m, c.empty() ? nullptr : &c[0], c.size(), &sat));
		for (size_t i = 0; i < c.size(); ++i)
			counts[i] += c[i];
		return sat;
	}

	// calcProbSingleFrame (MIBloomFilter.hpp:65-77), computed by the library in the reference's order of operations
	static inline double calcProbSingleFrame(double occupancy, unsigned hashNum, double freq, unsigned allowedMisses)
	{
		return btlbf_mibf_prob_single_frame(occupancy, hashNum, freq, allowedMisses);
	}

	// calcFrameProbs (MIBloomFilter.hpp:664-679): frameProbs is preallocated to the number of ids + 1; entries 1.. are
	// written, entry 0 is left as it is; returns the proportion of saturated entries.  Where the reference has undefined
	// behaviour (an id in the array beyond frameProbs, allowedMiss above the hash count, no entry with an id) this is an
	// error (btlbf_mibf_frame_probs).
	double calcFrameProbs(std::vector<double>& frameProbs, unsigned allowedMiss) const
	{
		double satProp = 0.0;
		btlbf_shim::check(btlbf_mibf_frame_probs(m_m, allowedMiss, frameProbs.empty() ? nullptr : &frameProbs[0],
		                                         frameProbs.size(), &satProp));
		return satProp;
	}

	// the whole ID array (getData of every rank)
	std::vector<T> getData() const
	{
		std::vector<T> d(getPop());
		btlbf_shim::check(btlbf_mibf_download(m_m, d.empty() ? nullptr : &d[0]));
		return d;
	}
	void setData(const std::vector<T>& d) { btlbf_shim::check(btlbf_mibf_upload(m_m, d.empty() ? nullptr : &d[0])); }
	std::vector<T> getCounts() const
	{
		std::vector<T> d(getPop());
		btlbf_shim::check(btlbf_mibf_download_counts(m_m, d.empty() ? nullptr : &d[0]));
		return d;
	}

	void store(const std::string& filterFilePath) const { btlbf_shim::check(btlbf_mibf_store(m_m, filterFilePath.c_str())); }

	// insertMIBF of every sequence (one id each, in sequence order) of a host buffer of reads of read_len bases
	void insertIDs(const std::string& seqs, unsigned readLen, const std::vector<uint32_t>& ids)
	{
		btlbf_layout l = layout(readLen);
		btlbf_shim::check(btlbf_mibf_insert_ids_seqs(m_m, seqs.data(), seqs.size(), &l, ids.data(), BTLBF_HOST, nullptr));
	}

	// insertSaturation; returns {clean windows, found, mutated, saturated}
	std::vector<uint64_t> insertSaturation(const std::string& seqs, unsigned readLen, const std::vector<uint32_t>& ids,
	                                       bool serial = false)
	{
		btlbf_layout l = layout(readLen);
		std::vector<uint64_t> c(4, 0);
		btlbf_shim::check(btlbf_mibf_saturate_seqs(m_m, seqs.data(), seqs.size(), &l, ids.data(),
		                                           serial ? BTLBF_ORDER_SERIAL : BTLBF_ORDER_PARALLEL, &c[0], BTLBF_HOST,
		                                           nullptr));
		return c;
	}

	// getMatchSignature of every window: values[len * h] raw T (0 at misses), match bitmap; returns the matched windows
	uint64_t query(const std::string& seqs, unsigned maxMiss, std::vector<T>& values, std::vector<uint64_t>& matchBits)
	{
		values.assign(seqs.size() * getHashNum() + 1, 0);
		matchBits.assign((seqs.size() + 63) / 64 + 1, 0);
		uint64_t c[2] = {0, 0};
		btlbf_shim::check(btlbf_mibf_query_seqs(m_m, seqs.data(), seqs.size(), nullptr, maxMiss, &values[0], &matchBits[0],
		                                        nullptr, c, BTLBF_HOST, nullptr));
		values.resize(seqs.size() * getHashNum());
		return c[1];
	}

	btlbf_mibf* handle() const { return m_m; }

  private:
	btlbf_mibf* m_m = nullptr;
	explicit MIBloomFilter(btlbf_mibf* m) : m_m(m) {}

	std::vector<uint64_t> stats() const
	{
		std::vector<uint64_t> s(3, 0);
		btlbf_shim::check(btlbf_mibf_stats(m_m, &s[0]));
		return s;
	}
	static btlbf_layout layout(unsigned readLen)
	{
		btlbf_layout l;
		l.starts = nullptr;
		l.n_seqs = 0;
		l.read_len = readLen;
		return l;
	}
};

} // namespace btlbf
#endif
