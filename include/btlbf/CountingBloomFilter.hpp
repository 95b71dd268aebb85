// include/btlbf/CountingBloomFilter.hpp -- drop-in for the reference's `CountingBloomFilter<T>`
// (/root/reference/CountingBloomFilter.hpp:26-111) with T = uint8_t, uint16_t, uint32_t or uint64_t, counters resident
// in HBM.  The kind of the C ABI follows sizeof(T) (BTLBF_COUNTING8 / 16 / 32 / 64); size() = sizeInBytes() / sizeof(T).
//
// Same constructors and method names; `U` is any indexable holder of m_hashNum hash values, as in
// the reference.  Per-k-mer calls apply in call order (BTLBF_ORDER_SERIAL on one row), so a
// single-threaded caller gets exactly the reference's counters; the batch members run in parallel
// (incrementAll stays exact; insert = incrementMin is order-dependent in the reference too).
// Threads: per-k-mer calls may come from many threads at once, as in the reference
// (CountingBloomFilter.hpp:117-132); they are serialised by the filter's lock inside the C ABI.
// Not reproduced: loadFilter's resize to sizeInBytes *elements* (CountingBloomFilter.hpp:275), an
// over-allocation that only matters for T wider than a byte.  Where the reference would silently misread a file whose
// header does not fit T (BloomFilterSize * sizeof(T) != BloomFilterSizeInBytes), loading fails here.
#ifndef BTLBF_COUNTINGBLOOMFILTER_HPP
#define BTLBF_COUNTINGBLOOMFILTER_HPP
#include "BloomFilter.hpp"
#include "detail.hpp"

#include <algorithm>
#include <cmath>
#include <istream>
#include <string>
#include <type_traits>
#include <vector>

template<typename T>
class CountingBloomFilter
{
	static_assert(sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8,
	              "the MI355X engine implements 8-, 16-, 32- and 64-bit counters");
	static constexpr int kKind = sizeof(T) == 1   ? BTLBF_COUNTING8
	                             : sizeof(T) == 2 ? BTLBF_COUNTING16
	                             : sizeof(T) == 4 ? BTLBF_COUNTING32
	                                              : BTLBF_COUNTING64;

  public:
	CountingBloomFilter() = default;
	CountingBloomFilter(size_t sizeInBytes, unsigned hashNum, unsigned kmerSize, unsigned countThreshold)
	{
		btlbf_shim::check(btlbf_create(&m_f, kKind, sizeInBytes, hashNum, kmerSize, countThreshold,
		                               btlbf_shim::default_device()));
	}
	CountingBloomFilter(const std::string& path, unsigned countThreshold)
	  : m_threshold(countThreshold)
	{
		loadFilter(path);
	}
	~CountingBloomFilter() { btlbf_destroy(m_f); }
	CountingBloomFilter(const CountingBloomFilter&) = delete;
	CountingBloomFilter& operator=(const CountingBloomFilter&) = delete;

	T operator[](size_t i)
	{
		T v = 0;
		btlbf_shim::check(btlbf_download(m_f, &v, i * sizeof(T), sizeof(T)));
		return v;
	}

	template<typename U>
	T minCount(const U& hashes) const // CountingBloomFilter.hpp:53-64
	{
		if (sizeof(T) == 1) {
			uint8_t v = 0;
			btlbf_shim::check(btlbf_min_count_hashes(m_f, row(hashes), 1, &v, BTLBF_HOST, nullptr));
			return (T)v;
		}
		T w = 0; // the full-width minimum
		btlbf_shim::check(btlbf_min_count_hashes_wide(m_f, row(hashes), 1, &w, BTLBF_HOST, nullptr));
		return w;
	}
	template<typename U>
	bool contains(const U& hashes) const // :190-196
	{
		uint8_t v = 0;
		btlbf_shim::check(btlbf_contains_hashes(m_f, row(hashes), 1, &v, BTLBF_HOST, nullptr));
		return v != 0;
	}
	template<typename U>
	void insert(const U& hashes) // :198-204
	{
		incrementMin(hashes);
	}
	template<typename U>
	bool insertAndCheck(const U& hashes) // :206-214
	{
		uint8_t v = 0;
		btlbf_shim::check(btlbf_insert_and_check_hashes(m_f, row(hashes), 1, &v, BTLBF_ORDER_SERIAL, BTLBF_HOST,
		                                                nullptr));
		return v != 0;
	}
	template<typename U>
	void incrementMin(const U& hashes) // :135-162
	{
		btlbf_shim::check(btlbf_insert_hashes(m_f, row(hashes), 1, BTLBF_INCREMENT_MIN, BTLBF_ORDER_SERIAL,
		                                      BTLBF_HOST, nullptr));
	}
	template<typename U>
	void incrementAll(const U& hashes) // :165-183
	{
		btlbf_shim::check(btlbf_insert_hashes(m_f, row(hashes), 1, BTLBF_INCREMENT_ALL, BTLBF_ORDER_SERIAL,
		                                      BTLBF_HOST, nullptr));
	}

	// ---- batch interface (fast path) ----
	void insertSeq(const std::string& seq, bool incrementAllCounters = false, bool serialOrder = false)
	{
		btlbf_shim::check(btlbf_insert_seqs(m_f, seq.data(), seq.size(), nullptr,
		                                    incrementAllCounters ? BTLBF_INCREMENT_ALL : BTLBF_INCREMENT_MIN,
		                                    serialOrder ? BTLBF_ORDER_SERIAL : BTLBF_ORDER_PARALLEL, BTLBF_HOST,
		                                    nullptr));
	}
	void containsSeq(const std::string& seq, std::vector<bool>& result, std::vector<bool>& valid) const
	{
		const size_t nw = (seq.size() + 63) / 64;
		std::vector<uint64_t> hb(nw ? nw : 1), vb(nw ? nw : 1);
		btlbf_shim::check(btlbf_contains_seqs(m_f, seq.data(), seq.size(), nullptr, hb.data(), vb.data(),
		                                      nullptr, BTLBF_HOST, nullptr));
		result.assign(seq.size(), false);
		valid.assign(seq.size(), false);
		for (size_t p = 0; p < seq.size(); ++p) {
			result[p] = btlbf_shim::bit(hb.data(), p);
			valid[p] = btlbf_shim::bit(vb.data(), p);
		}
	}

	unsigned getKmerSize() const { return btlbf_kmer_size(m_f); }
	unsigned getHashNum() const { return btlbf_hash_num(m_f); }
	unsigned threshold() const { return btlbf_threshold(m_f); }
	size_t size() const { return btlbf_size(m_f); }
	size_t sizeInBytes() const { return btlbf_size_bytes(m_f); }
	size_t popCount() const // :217-228
	{
		uint64_t v = 0;
		btlbf_shim::check(btlbf_popcount(m_f, &v));
		return v;
	}
	size_t filtered_popcount() const // :231-242
	{
		uint64_t v = 0;
		btlbf_shim::check(btlbf_filtered_popcount(m_f, &v));
		return v;
	}
	double FPR() const { return std::pow((double)popCount() / (double)size(), getHashNum()); }
	double filtered_FPR() const { return std::pow((double)filtered_popcount() / (double)size(), getHashNum()); }

	void loadFilter(const std::string& path) // :268-280
	{
		btlbf_destroy(m_f);
		m_f = nullptr;
		btlbf_shim::check(btlbf_load(&m_f, kKind, path.c_str(), m_threshold, btlbf_shim::default_device()));
	}
	// loadHeader(std::istream&), CountingBloomFilter.hpp:84,282-330: the header lines up to "[HeaderEnd]" -> a zeroed
	// filter of that geometry; the stream is left at the body (loadBody)
	void loadHeader(std::istream& file)
	{
		std::string text, line;
		while (std::getline(file, line)) {
			text += line + "\n";
			if (line == "[HeaderEnd]" || text.size() > (1u << 16))
				break;
		}
		btlbf_destroy(m_f);
		m_f = nullptr;
		btlbf_shim::check(btlbf_create_from_header(&m_f, kKind, text.data(), text.size(), m_threshold,
		                                           btlbf_shim::default_device()));
	}
	void loadBody(std::istream& file)
	{
		std::vector<char> chunk(1u << 24);
		const uint64_t total = sizeInBytes();
		for (uint64_t off = 0; off < total; off += chunk.size()) {
			const uint64_t n = std::min<uint64_t>(chunk.size(), total - off);
			file.read(chunk.data(), (std::streamsize)n);
			if ((uint64_t)file.gcount() != n) {
				std::cerr << "error: short read of the filter body" << std::endl;
				std::exit(EXIT_FAILURE);
			}
			btlbf_shim::check(btlbf_upload(m_f, chunk.data(), off, n));
		}
	}
	void storeFilter(const std::string& path) const // :331-342
	{
		std::cerr << "Writing a " << sizeInBytes() << " byte filter to " << path << " on disk.\n";
		btlbf_shim::check(btlbf_store(m_f, path.c_str()));
	}
	void storeHeader(std::ostream& out) const // :344-368
	{
		char buf[1024];
		size_t n = 0;
		btlbf_shim::check(btlbf_header(m_f, buf, sizeof buf, &n));
		out.write(buf, (std::streamsize)n);
	}
	friend std::ostream& operator<<(std::ostream& out, const CountingBloomFilter& bloom) // :371-379
	{
		bloom.storeHeader(out);
		std::vector<char> body(bloom.sizeInBytes());
		btlbf_shim::check(btlbf_download(bloom.m_f, body.data(), 0, body.size()));
		out.write(body.data(), (std::streamsize)body.size());
		return out;
	}

	btlbf_filter* handle() const { return m_f; }

	// ---- filter algebra (btlbf_combine / btlbf_fold / btlbf_threshold_bits): not in the reference ----
	// this = this OP other(s), counter by counter, in one pass over HBM: BTLBF_COMBINE_ADD saturates at the maximum of T, as
	// incrementAll does (:165-183), so it gives what incrementAll of all the inputs into one filter leaves;
	// BTLBF_COMBINE_MAX, BTLBF_COMBINE_MIN.  Filters of the same size, hash count, k and seeds.
	// (These members are templates only so that an explicit instantiation of the class -- a program that wants none of them
	// -- does not need the algebra's entry points at link time; callers write m.merge(other), f.fold(2), c.toBloomFilter().)
	template<typename Same = T>
	void merge(const CountingBloomFilter<Same>& other, int op = BTLBF_COMBINE_ADD)
	{
		merge(std::vector<const CountingBloomFilter<Same>*>{ &other }, op);
	}
	template<typename Same = T>
	void merge(const std::vector<const CountingBloomFilter<Same>*>& others, int op = BTLBF_COMBINE_ADD)
	{
		static_assert(std::is_same<Same, T>::value, "merge: counters of the same type");
		std::vector<btlbf_filter*> hs;
		for (const CountingBloomFilter<Same>* o : others)
			hs.push_back(o->m_f);
		btlbf_shim::check(btlbf_combine(m_f, hs.data(), (unsigned)hs.size(), op, nullptr));
	}
	// the filter of size() / factor counters: for counters built with incrementAll, the filter the same calls would have
	// built at that size; for insert (= incrementMin) an upper bound of it
	template<typename Same = T>
	CountingBloomFilter<Same> fold(uint64_t factor) const
	{
		static_assert(std::is_same<Same, T>::value, "fold: counters of the same type");
		btlbf_filter* h = nullptr;
		btlbf_shim::check(btlbf_fold(&h, m_f, factor));
		return CountingBloomFilter(h, m_threshold);
	}
	// the bit filter of the counters >= threshold (0: this filter's own): its contains() is this filter's at that
	// threshold (:190-196), in 1 / (8 sizeof(T)) of the memory
	template<typename Bits = BloomFilter>
	Bits toBloomFilter(unsigned threshold = 0) const
	{
		btlbf_filter* h = nullptr;
		btlbf_shim::check(btlbf_threshold_bits(&h, m_f, threshold));
		return Bits(h, typename Bits::AdoptHandle{});
	}

  private:
	CountingBloomFilter(btlbf_filter* owned, unsigned countThreshold)
	  : m_f(owned)
	  , m_threshold(countThreshold)
	{}

	// the first m_hashNum values of any indexable holder as a contiguous row.  A value, not a member: the
	// reference's per-k-mer calls may come from many threads at once (CountingBloomFilter.hpp:117-132)
	struct Row {
		std::vector<uint64_t> v;
		operator const uint64_t*() const { return v.data(); }
	};
	template<typename U>
	Row row(const U& hashes) const
	{
		Row r;
		const unsigned h = getHashNum();
		r.v.resize(h);
		for (unsigned i = 0; i < h; ++i)
			r.v[i] = hashes[i];
		return r;
	}

	btlbf_filter* m_f = nullptr;
	unsigned m_threshold = 0;
};

#endif
