// csrc/algebra_swar.hpp -- the arithmetic of the filter algebra (algebra_kernels.hip) on one 64-bit word that holds 8, 4,
// 2 or 1 counters: saturating add, maximum, minimum, non-zero count and ">= t", without unpacking to a counter per
// register.  Plain C++ that compiles for the host too, so that a stand-alone test can walk every pair of byte values
// (tests/cpp/test_fold_plan.cpp).  BYTES is the counter's width.
//
// With H the top bit of every counter and L the rest, (a & L) + (b & L) cannot carry from one counter into the next; its
// top bit is the carry into the counter's top bit, and the carry OUT of a counter is the majority of that and the two
// top bits.  A carry-out bit shifted down to the counter's bit 0 and multiplied by the counter's all-ones spreads to the
// whole counter (the products do not overlap) -- that is the saturation mask, and likewise the ">=" mask of max / min.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BTLBF_HD __host__ __device__ __forceinline__
#else
#define BTLBF_HD inline
#endif

namespace btlbf {

template <int BYTES>
struct Swar {
	static_assert(BYTES == 1 || BYTES == 2 || BYTES == 4, "counters of 1, 2 or 4 bytes share a word");
	static constexpr int kBits = 8 * BYTES;
	static constexpr uint64_t kOnes = BYTES == 4 ? 0xffffffffull : BYTES == 2 ? 0xffffull : 0xffull; // one counter's MAX
	static constexpr uint64_t kLsb = ~0ull / kOnes;                                                   // bit 0 of every counter
	static constexpr uint64_t H = kLsb << (kBits - 1), L = ~H;

	// a mask bit at every counter's top bit -> all ones over those counters
	static BTLBF_HD uint64_t spread(uint64_t top) { return (top >> (kBits - 1)) * kOnes; }
	// min(a + b, MAX) per counter (incrementAll's saturation, CountingBloomFilter.hpp:165-183)
	static BTLBF_HD uint64_t add_sat(uint64_t a, uint64_t b)
	{
		const uint64_t t = (a & L) + (b & L);
		const uint64_t sum = t ^ ((a ^ b) & H);
		const uint64_t carry = ((a & b) | ((a | b) & t)) & H;
		return sum | spread(carry);
	}
	// all ones over the counters with a >= b
	static BTLBF_HD uint64_t ge_mask(uint64_t a, uint64_t b)
	{
		const uint64_t t = (a | H) - (b & L); // top bit: the low parts compare a >= b; no borrow leaves a counter
		return spread(((a & ~b) | (~(a ^ b) & t)) & H);
	}
	static BTLBF_HD uint64_t max(uint64_t a, uint64_t b)
	{
		const uint64_t m = ge_mask(a, b);
		return (a & m) | (b & ~m);
	}
	static BTLBF_HD uint64_t min(uint64_t a, uint64_t b)
	{
		const uint64_t m = ge_mask(a, b);
		return (b & m) | (a & ~m);
	}
	// a bit at the top of every counter that is not zero
	static BTLBF_HD uint64_t nonzero_top(uint64_t v) { return (((v & L) + L) | v) & H; }
};

// 64-bit counters: one per word; the saturation is the carry out of the word (of its high half, in the ISA)
template <>
struct Swar<8> {
	static BTLBF_HD uint64_t add_sat(uint64_t a, uint64_t b)
	{
		const uint64_t s = a + b;
		return s < a ? ~0ull : s;
	}
	static BTLBF_HD uint64_t max(uint64_t a, uint64_t b) { return a >= b ? a : b; }
	static BTLBF_HD uint64_t min(uint64_t a, uint64_t b) { return a >= b ? b : a; }
	static BTLBF_HD uint64_t ge_mask(uint64_t a, uint64_t b) { return a >= b ? ~0ull : 0; }
	static BTLBF_HD uint64_t nonzero_top(uint64_t v) { return v ? 1ull << 63 : 0; }
};

// The low `n` bytes of a 16-byte vector (w0 = bytes 0..7, w1 = bytes 8..15), n in 0..16: what of a slice's last vector
// belongs to the slice (fold_kernel)
BTLBF_HD void keep_low_bytes(uint64_t& w0, uint64_t& w1, uint32_t n)
{
	if (n < 8) {
		w0 &= n ? ~0ull >> (64 - 8 * n) : 0;
		w1 = 0;
	} else if (n < 16) {
		w1 &= n > 8 ? ~0ull >> (64 - 8 * (n - 8)) : 0;
	}
}

// 16 bytes from byte `shift` (0..15) of the 32 bytes a0 a1 b0 b1 (little-endian words, a before b): the unaligned read of a
// slice, from the two aligned vectors around it.  A funnel shift over 64-bit words.
BTLBF_HD void align_bytes(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1, uint32_t shift, uint64_t& w0, uint64_t& w1)
{
	const bool up = shift >= 8;
	const uint64_t x = up ? a1 : a0, y = up ? b0 : a1, z = up ? b1 : b0;
	const uint32_t bits = 8 * (shift & 7);
	w0 = bits ? (x >> bits) | (y << (64 - bits)) : x;
	w1 = bits ? (y >> bits) | (z << (64 - bits)) : y;
}

} // namespace btlbf
