// oracle/standin/sdsl/bit_vector_il.hpp -- STAND-IN, TEST INFRASTRUCTURE ONLY.
// Not sdsl-lite: the few names the reference's miBF headers use from it (MIBloomFilter.hpp, MIBFConstructSupport.hpp),
// written from those call sites so that the genuine miBF code compiles behind oracle/ref_mibf_driver.cpp where
// sdsl-lite is not installed.  Semantics as sdsl-lite documents them: bit i is bit i%64 of word i/64, and
// rank_support_il<1>(i) is the number of set bits in [0, i) (exclusive).
#ifndef BTLBF_STANDIN_SDSL_BIT_VECTOR_IL_HPP
#define BTLBF_STANDIN_SDSL_BIT_VECTOR_IL_HPP
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace sdsl {

// plain bit vector: zeroed, size() in bits, data() = its 64-bit words
class bit_vector
{
  public:
	bit_vector()
	  : m_size(0)
	{}
	explicit bit_vector(size_t bits)
	  : m_size(bits)
	  , m_words((bits + 63) / 64, 0)
	{}
	size_t size() const { return m_size; }
	uint64_t* data() { return m_words.data(); }
	const uint64_t* data() const { return m_words.data(); }

  private:
	size_t m_size;
	std::vector<uint64_t> m_words;
};

// "interleaved" bit vector: here simply a copy of the words (the interleaving is a storage detail)
template<uint32_t t_bs = 512>
class bit_vector_il
{
  public:
	bit_vector_il()
	  : m_size(0)
	{}
	bit_vector_il(const bit_vector& bv)
	  : m_size(bv.size())
	  , m_words(bv.data(), bv.data() + (bv.size() + 63) / 64)
	{}
	size_t size() const { return m_size; }
	bool operator[](size_t i) const { return (m_words[i >> 6] >> (i & 63)) & 1; }
	const std::vector<uint64_t>& words() const { return m_words; }

  private:
	size_t m_size;
	std::vector<uint64_t> m_words;
};

// rank over a bit_vector_il: operator()(i) = set bits in [0, i), 0 <= i <= size()
template<uint8_t t_b = 1, uint32_t t_bs = 512>
class rank_support_il
{
  public:
	rank_support_il()
	  : m_v(NULL)
	{}
	explicit rank_support_il(const bit_vector_il<t_bs>* v)
	  : m_v(v)
	  , m_before(1, 0)
	{
		const std::vector<uint64_t>& w = v->words();
		for (size_t i = 0; i < w.size(); ++i)
			m_before.push_back(m_before.back() + (uint64_t)__builtin_popcountll(w[i]));
	}
	uint64_t operator()(size_t i) const
	{
		const uint64_t part = (i & 63) ? m_v->words()[i >> 6] & ((uint64_t(1) << (i & 63)) - 1) : 0;
		return m_before[i >> 6] + (uint64_t)__builtin_popcountll(part);
	}

  private:
	const bit_vector_il<t_bs>* m_v;
	std::vector<uint64_t> m_before; // set bits before word i
};

// the .sdsl side file is not written or read here
template<class V>
bool
store_to_file(const V&, const std::string&)
{
	return true;
}
template<class V>
bool
load_from_file(V&, const std::string&)
{
	return true;
}

} // namespace sdsl
#endif
