// tests/cpp/ref_wide_counter_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// The genuine reference's CountingBloomFilter<T> for T = uint16_t, uint32_t, uint64_t, for
// tests/test_wide_counter_vs_ref.py: a program around the reference's CountingBloomFilter.hpp and
// vendor/ntHashIterator.hpp, compiled by the test from where those headers lie (never copied here).  Built with
// -fno-access-control: a prefilled body goes straight into m_filter.
//
// Input (a text file, argv[1]), one case after another until the end of the file; a case is
//   bits sizeInBytes h k threshold op(min|all|check) n_reads
//   the body before the call as hex (sizeInBytes rounded up to 8, two digits per byte), or "-" for zeros
//   n_reads lines, one read each
// and `out_path` (argv[2]) is where every case's filter is stored (storeFilter) and read back from.
// Output per case:
//   "size <size()> <sizeInBytes()>", "body <hex>", "out <one 0/1 per clean k-mer>" (check only, else "out -"),
//   "min <minCount of every clean k-mer after the call>", "pop <popCount()> <filtered_popcount()>",
//   "file <hex of the stored file>", "reload <1 if the file loads to the same counters>"
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "vendor/ntHashIterator.hpp"

#include "CountingBloomFilter.hpp"

namespace {

void hex_out(const char* tag, const unsigned char* p, size_t n)
{
	std::string s(tag);
	static const char* d = "0123456789abcdef";
	for (size_t i = 0; i < n; ++i) {
		s.push_back(d[p[i] >> 4]);
		s.push_back(d[p[i] & 15]);
	}
	std::cout << s << "\n";
}

template<typename T>
void run_case(size_t nbytes, unsigned h, unsigned k, unsigned thr, const std::string& op, const std::string& body,
              const std::vector<std::string>& reads, const char* out_path)
{
	CountingBloomFilter<T> f(nbytes, h, k, thr);
	if (body != "-") {
		unsigned char* raw = reinterpret_cast<unsigned char*>(f.m_filter.data());
		for (size_t i = 0; i < f.sizeInBytes(); ++i)
			raw[i] = (unsigned char)std::stoul(body.substr(2 * i, 2), nullptr, 16);
	}
	std::string out;
	for (const std::string& s : reads) {
		ntHashIterator it(s, h, k);
		while (it != it.end()) {
			if (op == "min")
				f.insert(*it);
			else if (op == "all")
				f.incrementAll(*it);
			else
				out.push_back(f.insertAndCheck(*it) ? '1' : '0');
			++it;
		}
	}
	std::cout << "size " << f.size() << " " << f.sizeInBytes() << "\n";
	hex_out("body ", reinterpret_cast<const unsigned char*>(f.m_filter.data()), f.sizeInBytes());
	std::cout << "out " << (op == "check" && !out.empty() ? out : "-") << "\n";
	std::cout << "min";
	for (const std::string& s : reads) {
		ntHashIterator it(s, h, k);
		while (it != it.end()) {
			std::cout << " " << (unsigned long long)f.minCount(*it);
			++it;
		}
	}
	std::cout << "\npop " << f.popCount() << " " << f.filtered_popcount() << "\n";
	f.storeFilter(out_path);
	std::ifstream in(out_path, std::ios::binary);
	std::vector<unsigned char> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
	hex_out("file ", file.data(), file.size());
	CountingBloomFilter<T> g(out_path, thr);
	bool same = g.size() == f.size() && g.sizeInBytes() == f.sizeInBytes();
	for (size_t i = 0; same && i < f.size(); ++i)
		same = g[i] == f[i];
	std::cout << "reload " << (same ? 1 : 0) << "\n";
}

} // namespace

int main(int argc, char** argv)
{
	if (argc != 3)
		return 2;
	std::ifstream in(argv[1]);
	unsigned bits, h, k, thr;
	size_t nbytes, n_reads;
	std::string op, body;
	while (in >> bits >> nbytes >> h >> k >> thr >> op >> n_reads >> body) {
		std::vector<std::string> reads(n_reads);
		for (std::string& s : reads)
			in >> s;
		if (bits == 16)
			run_case<uint16_t>(nbytes, h, k, thr, op, body, reads, argv[2]);
		else if (bits == 32)
			run_case<uint32_t>(nbytes, h, k, thr, op, body, reads, argv[2]);
		else if (bits == 64)
			run_case<uint64_t>(nbytes, h, k, thr, op, body, reads, argv[2]);
		else
			return 3;
	}
	return 0;
}
