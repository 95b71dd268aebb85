// oracle/ref_mibf_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// The second unit of oracle/_ref/libbtlref.so (see ref_driver.cpp for the rules): extern "C" entry points around the
// GENUINE reference miBF headers, compiled from where they lie (never copied into this repo):
//   MIBFConstructSupport<T, H> (MIBFConstructSupport.hpp:36-148): insertBV, getEmptyMIBF, insertMIBF, insertSaturation
//   MIBloomFilter<T>           (MIBloomFilter.hpp): size, getPop, getData, getPopNonZero, getPopSaturated, getIDCounts,
//                              both atRank overloads, store
// for T = uint16_t / uint32_t and H = ntHashIterator / stHashIterator (seeds, h2 = 1).
// sdsl-lite and google sparsehash, which those headers include, are replaced by the stand-ins of oracle/standin/ (this
// unit alone gets -Istandin): a rank that counts the ones of [0, i) and a hash set that walks in ascending order.
// MIBFQuerySupport.hpp (needs boost) is not used; the atRank rule it rests on is called directly.
// Only public members are used.  The private m_counts shows through the data array after insertSaturation (the
// largest-count choice); the bit vector through atRank.
//
// Include order matters.  MIBloomFilter.hpp:107 says `#pragma pack(1)` for its FileHeader and never resets it, so every
// type first DEFINED after that line in this unit is laid out without padding: MIBFConstructSupport itself (its own
// business: x86 reads its misaligned members), but also any standard or vendor header first seen after it.  A packed
// std::_Rb_tree_node_base does not match the one libstdc++'s compiled rebalancing code expects -- a driver that lets
// <set> come in through google/dense_hash_set faults inside values.insert (MIBFConstructSupport.hpp:116) -- and a
// packed stHashIterator does not match the one ref_driver.cpp's unit compiled into the same library.  So: everything
// the reference headers, the stand-ins and this file need comes first, with the default layout; the packing is reset
// after the reference headers for the code below.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iostream>
#include <random> // std::minstd_rand, which MIBloomFilter.hpp uses without including it
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "vendor/ntHashIterator.hpp"
#include "vendor/stHashIterator.hpp"

#include "MIBFConstructSupport.hpp"
#pragma pack()

namespace {

struct Base
{
	virtual ~Base() {}
	virtual uint64_t filter_size() const = 0;
	virtual void insert_bv(const std::string& s) = 0;
	virtual void get_empty() = 0;
	virtual void insert_mibf(const std::string& s, uint32_t id) = 0;
	virtual void insert_saturation(const std::string& s, uint32_t id) = 0;
	virtual void stats(uint64_t* out4) const = 0;
	virtual void bits(uint8_t* out) const = 0;
	virtual void data(uint32_t* out) const = 0;
	virtual uint64_t id_counts(uint64_t* out, size_t n) const = 0;
	virtual size_t at_rank(const std::string&, unsigned, uint64_t*, uint8_t*, uint32_t*, uint32_t*, uint8_t*, uint32_t*, size_t) const = 0;
	virtual void store(const std::string& path) const = 0;
};

template<typename T, class H>
struct Impl : public Base
{
	// members in this order: MIBFConstructSupport keeps a REFERENCE to the seed vector (MIBFConstructSupport.hpp:158),
	// so the vector is a named member that outlives it
	const std::vector<std::string> seeds;
	const std::vector<std::vector<unsigned> > parsed;
	const unsigned k, h;
	MIBFConstructSupport<T, H> cs;
	MIBloomFilter<T>* mi;
	bool sat_called;

	Impl(size_t entries, unsigned k_, unsigned h_, double occupancy, const std::vector<std::string>& ss)
	  : seeds(ss)
	  , parsed(stHashIterator::parseSeed(ss))
	  , k(k_)
	  , h(h_)
	  , cs(entries, k_, h_, occupancy, seeds)
	  , mi(NULL)
	  , sat_called(false)
	{}

	~Impl()
	{
		// ~MIBFConstructSupport asserts that both stages ran (:48-50): run them over nothing where the caller did not
		get_empty();
		if (!sat_called)
			insert_saturation(std::string(), 0);
		delete mi;
	}

	// the iterator as the reference's callers construct it; the overload is chosen by H
	static ntHashIterator* make(const Impl& o, const std::string& s, ntHashIterator*) { return new ntHashIterator(s, o.h, o.k); }
	static stHashIterator* make(const Impl& o, const std::string& s, stHashIterator*)
	{
		return new stHashIterator(s, o.parsed, o.h, 1, o.k);
	}
	struct Itr // owns one iterator (stHashIterator has no copy constructor: never copied)
	{
		H* p;
		Itr(const Impl& o, const std::string& s)
		  : p(make(o, s, (H*)NULL))
		{}
		~Itr() { delete p; }
	};

	uint64_t filter_size() const { return cs.getFilterSize(); }
	void insert_bv(const std::string& s)
	{
		Itr it(*this, s);
		cs.insertBV(*it.p);
	}
	void get_empty()
	{
		if (!mi)
			mi = cs.getEmptyMIBF();
	}
	void insert_mibf(const std::string& s, uint32_t id)
	{
		Itr it(*this, s);
		cs.insertMIBF(*mi, *it.p, (T)id);
	}
	void insert_saturation(const std::string& s, uint32_t id)
	{
		Itr it(*this, s);
		cs.insertSaturation(*mi, *it.p, (T)id);
		sat_called = true;
	}
	void stats(uint64_t* out4) const
	{
		out4[0] = mi->size();
		out4[1] = mi->getPop();
		out4[2] = mi->getPopNonZero();
		out4[3] = mi->getPopSaturated();
	}
	// bit p of the bit vector, as atRank sees it (m_bv[hash % size], MIBloomFilter.hpp:504-515)
	void bits(uint8_t* out) const
	{
		std::vector<uint64_t> hv(h), rp(h);
		for (uint64_t p = 0; p < mi->size(); ++p) {
			for (unsigned i = 0; i < h; ++i)
				hv[i] = p;
			out[p] = mi->atRank(hv.data(), rp) ? 1 : 0;
		}
	}
	void data(uint32_t* out) const
	{
		const uint64_t n = mi->getPop();
		for (uint64_t r = 0; r < n; ++r)
			out[r] = mi->getData(r);
	}
	uint64_t id_counts(uint64_t* out, size_t n) const
	{
		std::vector<size_t> c(n, 0);
		const uint64_t sat = mi->getIDCounts(c);
		for (size_t i = 0; i < n; ++i)
			out[i] = c[i];
		return sat;
	}
	// per emitted window: pos; atRank(hashes, rankPos) -> ok0 and the data at rankPos (zeros when it fails);
	// atRank(hashes, rankPos, hits, maxMiss) -> the misses it returns, hits[] and the data at the hit positions
	size_t at_rank(
	    const std::string& s,
	    unsigned max_miss,
	    uint64_t* pos,
	    uint8_t* ok0,
	    uint32_t* vals0,
	    uint32_t* misses,
	    uint8_t* hits,
	    uint32_t* vals,
	    size_t cap) const
	{
		size_t n = 0;
		Itr it(*this, s);
		H& itr = *it.p;
		for (; itr != itr.end(); ++itr, ++n) {
			if (n >= cap)
				continue;
			pos[n] = itr.pos();
			std::vector<uint64_t> rp(h, 0);
			ok0[n] = mi->atRank(*itr, rp) ? 1 : 0;
			for (unsigned i = 0; i < h; ++i)
				vals0[n * h + i] = ok0[n] ? mi->getData(rp[i]) : 0;
			std::vector<uint64_t> rp2(h, 0);
			std::vector<bool> hit(h, false);
			misses[n] = mi->atRank(*itr, rp2, hit, max_miss);
			for (unsigned i = 0; i < h; ++i) {
				hits[n * h + i] = hit[i] ? 1 : 0;
				vals[n * h + i] = hit[i] ? mi->getData(rp2[i]) : 0;
			}
		}
		return n;
	}
	void store(const std::string& path) const { mi->store(path); }
};

Base*
B(void* p)
{
	return static_cast<Base*>(p);
}

} // namespace

extern "C"
{

	// nseeds == 0: ntHashIterator(seq, h, k); else stHashIterator over the seeds with h2 = 1 (h = nseeds)
	void* ref_mibf_new(
	    unsigned id_bytes,
	    uint64_t expected_entries,
	    unsigned k,
	    unsigned h,
	    double occupancy,
	    const char* const* seeds,
	    unsigned nseeds)
	{
		std::vector<std::string> ss;
		for (unsigned i = 0; i < nseeds; ++i)
			ss.push_back(seeds[i]);
		if (id_bytes != 2 && id_bytes != 4)
			return NULL;
		if (nseeds == 0)
			return id_bytes == 2 ? (Base*)new Impl<uint16_t, ntHashIterator>(expected_entries, k, h, occupancy, ss)
			                     : (Base*)new Impl<uint32_t, ntHashIterator>(expected_entries, k, h, occupancy, ss);
		if (nseeds != h)
			return NULL;
		return id_bytes == 2 ? (Base*)new Impl<uint16_t, stHashIterator>(expected_entries, k, h, occupancy, ss)
		                     : (Base*)new Impl<uint32_t, stHashIterator>(expected_entries, k, h, occupancy, ss);
	}
	void ref_mibf_free(void* p) { delete B(p); }
	uint64_t ref_mibf_filter_size(void* p) { return B(p)->filter_size(); }
	void ref_mibf_insert_bv(void* p, const char* seq, size_t len) { B(p)->insert_bv(std::string(seq, len)); }
	void ref_mibf_get_empty(void* p) { B(p)->get_empty(); }
	void ref_mibf_insert_mibf(void* p, const char* seq, size_t len, uint32_t id)
	{
		B(p)->insert_mibf(std::string(seq, len), id);
	}
	void ref_mibf_insert_saturation(void* p, const char* seq, size_t len, uint32_t id)
	{
		B(p)->insert_saturation(std::string(seq, len), id);
	}
	// out4 = {size(), getPop(), getPopNonZero(), getPopSaturated()}
	void ref_mibf_stats(void* p, uint64_t* out4) { B(p)->stats(out4); }
	void ref_mibf_bits(void* p, uint8_t* out_size) { B(p)->bits(out_size); }
	void ref_mibf_data(void* p, uint32_t* out_pop) { B(p)->data(out_pop); }
	uint64_t ref_mibf_id_counts(void* p, uint64_t* out_n, size_t n) { return B(p)->id_counts(out_n, n); }
	size_t ref_mibf_at_rank(
	    void* p,
	    const char* seq,
	    size_t len,
	    unsigned max_miss,
	    uint64_t* pos,
	    uint8_t* ok0,
	    uint32_t* vals0,
	    uint32_t* misses,
	    uint8_t* hits,
	    uint32_t* vals,
	    size_t cap)
	{
		return B(p)->at_rank(std::string(seq, len), max_miss, pos, ok0, vals0, misses, hits, vals, cap);
	}
	void ref_mibf_store(void* p, const char* path) { B(p)->store(std::string(path)); }

} // extern "C"
