// tests/cpp/test_wide_shim_link.cpp -- TEST-ONLY: CountingBloomFilter<T> of include/btlbf/ instantiated whole for
// T = uint16_t, uint32_t, uint64_t (and uint8_t, as before), member templates included, and linked against the stub ABI
// (tests/cpp/stub_abi.cpp + stub_abi_wide.cpp).  No GPU: main() only constructs and destroys a filter of each width on
// the stub, whose geometry getters are the stub's own.
#include "btlbf/CountingBloomFilter.hpp"

#include <cstdio>
#include <sstream>
#include <type_traits>
#include <vector>

template class CountingBloomFilter<uint8_t>;
template class CountingBloomFilter<uint16_t>;
template class CountingBloomFilter<uint32_t>;
template class CountingBloomFilter<uint64_t>;

// every member template with a holder of hash values; never called (the stub computes nothing wide)
template<typename T>
T use_all(CountingBloomFilter<T>& f, const std::vector<uint64_t>& hv)
{
	static_assert(std::is_same<decltype(f.minCount(hv)), T>::value, "minCount returns the full-width T");
	static_assert(std::is_same<decltype(f[0]), T>::value, "operator[] returns the full-width T");
	f.insert(hv);
	f.incrementMin(hv);
	f.incrementAll(hv);
	std::ostringstream os;
	os << f;
	return (T)(f.minCount(hv) + f[0] + f.contains(hv) + f.insertAndCheck(hv));
}
template uint16_t use_all<uint16_t>(CountingBloomFilter<uint16_t>&, const std::vector<uint64_t>&);
template uint32_t use_all<uint32_t>(CountingBloomFilter<uint32_t>&, const std::vector<uint64_t>&);
template uint64_t use_all<uint64_t>(CountingBloomFilter<uint64_t>&, const std::vector<uint64_t>&);

int main()
{
	CountingBloomFilter<uint16_t> a(64, 2, 8, 1);
	CountingBloomFilter<uint32_t> b(64, 2, 8, 1);
	CountingBloomFilter<uint64_t> c(64, 2, 8, 1);
	if (a.getHashNum() != 2 || b.getKmerSize() != 8 || c.getHashNum() != 2)
		return 1;
	std::printf("wide shim links\n");
	return 0;
}
