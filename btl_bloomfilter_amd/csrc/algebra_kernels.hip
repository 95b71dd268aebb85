// csrc/algebra_kernels.hip -- the filter algebra: streaming kernels that write a filter where the others (popcount,
// digest, compare: aux_kernels.hip) only read one.  combine_kernel: dst = dst OP s_1 OP ... OP s_n in one pass, with the
// result's popcount; fold_kernel: a filter of m positions into one of m / factor (positions are hash % m, so the result
// is the filter built at the smaller size); threshold_kernel: a counting filter into the bit filter of its counters
// >= t.  All three are HBM-bound: 16-byte non-temporal loads, 16-byte stores, a grid-stride loop; the arithmetic is on
// 64-bit words of packed counters (algebra_swar.hpp).
#include "internal.hpp"
#include "algebra_swar.hpp"
#include "../../include/btlbf.h"

namespace btlbf {

namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

struct Vec {
	uint64_t w0, w1;
};
__device__ __forceinline__ Vec load_vec(const void* base, uint64_t i)
{
	const v4u v = __builtin_nontemporal_load(static_cast<const v4u*>(base) + i);
	return Vec{((uint64_t)v.y << 32) | v.x, ((uint64_t)v.w << 32) | v.z};
}
__device__ __forceinline__ void store_vec(void* base, uint64_t i, const Vec& a)
{
	const v4u v = {(uint32_t)a.w0, (uint32_t)(a.w0 >> 32), (uint32_t)a.w1, (uint32_t)(a.w1 >> 32)};
	static_cast<v4u*>(base)[i] = v;
}

// one 64-bit word of a filter of CB-byte counters (CB == 0: bits) under a BTLBF_COMBINE_* op
template <int CB>
__device__ __forceinline__ uint64_t combine_word(int op, uint64_t a, uint64_t b)
{
	if constexpr (CB == 0) {
		return op == BTLBF_COMBINE_OR ? a | b : op == BTLBF_COMBINE_AND ? a & b : a & ~b;
	} else {
		using S = Swar<CB>;
		return op == BTLBF_COMBINE_ADD ? S::add_sat(a, b) : op == BTLBF_COMBINE_MAX ? S::max(a, b) : S::min(a, b);
	}
}
// set bits / non-zero counters of a word
template <int CB>
__device__ __forceinline__ uint32_t pop_word(uint64_t v)
{
	if constexpr (CB == 0)
		return __popcll(v);
	else
		return __popcll(Swar<CB>::nonzero_top(v));
}

// ---- combine --------------------------------------------------------------------------------------
// N is the number of sources the kernel loads (the pointers are kernel arguments, indexed by constants: scalar
// registers, no scratch), n <= N the number that count: the slots from n on repeat source 0, so that their loads are
// valid (and cached), and are not applied.  op is uniform.
template <int N>
struct CombinePtrs {
	const void* p[N];
};

template <int CB, int N>
__global__ __launch_bounds__(256) void combine_kernel(void* dst, CombinePtrs<N> src, uint32_t n, int op, uint64_t n_vec,
                                                      unsigned long long* pop)
{
	unsigned long long acc = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (uint64_t)gridDim.x * blockDim.x) {
		Vec d = load_vec(dst, i);
		Vec s[N];
#pragma unroll
		for (int j = 0; j < N; ++j)
			s[j] = load_vec(src.p[j], i);
#pragma unroll
		for (int j = 0; j < N; ++j) {
			if (j < (int)n) {
				d.w0 = combine_word<CB>(op, d.w0, s[j].w0);
				d.w1 = combine_word<CB>(op, d.w1, s[j].w1);
			}
		}
		store_vec(dst, i, d);
		acc += pop_word<CB>(d.w0) + pop_word<CB>(d.w1);
	}
	// wave reduce, then one atomic per wave (popcount_kernel)
	for (int o = 32; o > 0; o >>= 1)
		acc += __shfl_xor(acc, o, 64);
	if ((threadIdx.x & 63) == 0 && acc)
		atomicAdd(pop, acc);
}

template <int CB, int N>
hipError_t combine_n(int op, void* dst, const CombineSrcs& srcs, unsigned n, uint64_t n_vec, unsigned long long* pop,
                     hipStream_t s)
{
	CombinePtrs<N> p;
	for (int j = 0; j < N; ++j)
		p.p[j] = srcs.p[j < (int)n ? j : 0];
	uint64_t blocks = (n_vec + 255) / 256;
	if (blocks > 4096)
		blocks = 4096;
	hipLaunchKernelGGL((combine_kernel<CB, N>), dim3((unsigned)blocks), dim3(256), 0, s, dst, p, (uint32_t)n, op, n_vec, pop);
	return hipGetLastError();
}

template <int CB>
hipError_t combine_cb(int op, void* dst, const CombineSrcs& srcs, unsigned n, uint64_t n_vec, unsigned long long* pop,
                      hipStream_t s)
{
	if (n <= 1)
		return combine_n<CB, 1>(op, dst, srcs, n, n_vec, pop, s);
	if (n == 2)
		return combine_n<CB, 2>(op, dst, srcs, n, n_vec, pop, s);
	if (n == 3)
		return combine_n<CB, 3>(op, dst, srcs, n, n_vec, pop, s);
	if (n == 4)
		return combine_n<CB, 4>(op, dst, srcs, n, n_vec, pop, s);
	if (n <= 8)
		return combine_n<CB, 8>(op, dst, srcs, n, n_vec, pop, s);
	return combine_n<CB, 16>(op, dst, srcs, n, n_vec, pop, s);
}

// ---- fold -------------------------------------------------------------------------------------------
// One thread per 16-byte vector v of a result row, walking the row's slices.  Slice j's vector v starts at source byte
// j * stride + 16 v, at any alignment: ALIGNED (stride a multiple of 16) reads it as it lies; otherwise the two aligned
// vectors around it are loaded and shifted together (align_bytes) -- no misaligned address is ever cast to a vector type.
// The second one is loaded only where the slice reaches into it (else the first again: a valid address, and a load the
// compiler can issue early).  Of a slice's last vector only the slice's own bytes count (keep_low_bytes): behind them
// lies the next slice, or the array's padding.  So the result's padding comes out zero.
template <int CB, bool ALIGNED>
__global__ __launch_bounds__(256) void fold_kernel(const void* src, uint64_t stride, uint64_t valid, uint64_t n_slices,
                                                   uint64_t per_group, void* dst, uint64_t n_vec)
{
	const uint64_t g = blockIdx.y;
	const uint64_t j0 = g * per_group;
	const uint64_t j1 = j0 + per_group < n_slices ? j0 + per_group : n_slices;
	for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_vec; v += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t off = 16 * v;
		const uint32_t keep = valid >= off + 16 ? 16u : valid > off ? (uint32_t)(valid - off) : 0u;
		Vec acc{0, 0};
#pragma unroll 4
		for (uint64_t j = j0; j < j1; ++j) {
			const uint64_t a = j * stride + off;
			Vec x;
			if (ALIGNED) {
				x = load_vec(src, a >> 4);
			} else {
				const uint32_t sh = (uint32_t)a & 15;
				const uint64_t q = a >> 4;
				const Vec lo = load_vec(src, q), hi = load_vec(src, sh + keep > 16 ? q + 1 : q);
				align_bytes(lo.w0, lo.w1, hi.w0, hi.w1, sh, x.w0, x.w1);
			}
			keep_low_bytes(x.w0, x.w1, keep);
			if constexpr (CB == 0) {
				acc.w0 |= x.w0;
				acc.w1 |= x.w1;
			} else {
				acc.w0 = Swar<CB>::add_sat(acc.w0, x.w0);
				acc.w1 = Swar<CB>::add_sat(acc.w1, x.w1);
			}
		}
		store_vec(dst, g * n_vec + v, acc);
	}
}

template <int CB>
hipError_t fold_cb(const void* src, uint64_t stride, uint64_t valid, uint64_t n_slices, uint64_t per_group, uint64_t groups,
                   void* dst, uint64_t n_vec, hipStream_t s)
{
	uint64_t bx = (n_vec + 255) / 256;
	if (bx > 4096)
		bx = 4096;
	const dim3 grid((unsigned)bx, (unsigned)groups);
	if (stride % 16 == 0)
		hipLaunchKernelGGL((fold_kernel<CB, true>), grid, dim3(256), 0, s, src, stride, valid, n_slices, per_group, dst, n_vec);
	else
		hipLaunchKernelGGL((fold_kernel<CB, false>), grid, dim3(256), 0, s, src, stride, valid, n_slices, per_group, dst, n_vec);
	return hipGetLastError();
}

// ---- threshold ------------------------------------------------------------------------------------------
// A lane loads one vector of E = 16 / CB counters and makes E bits of it; the G = 64 / E lanes whose vectors make up one
// 64-bit word of the result OR their bits together (G divides the wave, and a group's lanes leave the loop together), and
// the group's first lane stores the whole word: no word is written by two lanes, no atomics, coalesced loads.  Vectors
// from src_n_vec on count as zero, so the last partial word and the result's padding come out zero.
template <int CB>
__global__ __launch_bounds__(256) void threshold_kernel(const void* src, uint64_t src_n_vec, uint64_t thr_word,
                                                        uint64_t* out, uint64_t out_words)
{
	constexpr int E = 16 / CB, G = 64 / E, W = 8 * CB;
	const uint64_t total = out_words * G;
	const uint32_t sub = threadIdx.x & (G - 1);
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
		Vec x{0, 0};
		if (i < src_n_vec)
			x = load_vec(src, i);
		const uint64_t m[2] = {Swar<CB>::ge_mask(x.w0, thr_word), Swar<CB>::ge_mask(x.w1, thr_word)};
		uint64_t bits = 0;
#pragma unroll
		for (int e = 0; e < E; ++e)
			bits |= ((m[e / (E / 2)] >> ((e % (E / 2)) * W)) & 1ull) << e;
		uint64_t w = bits << (E * sub);
#pragma unroll
		for (int o = 1; o < G; o <<= 1)
			w |= __shfl_xor(w, o, 64);
		if (sub == 0)
			out[i / G] = w;
	}
}

template <int CB>
hipError_t threshold_cb(const void* src, uint64_t src_n_vec, uint64_t threshold, void* out, uint64_t out_words,
                        hipStream_t s)
{
	uint64_t thr_word; // the threshold in every counter of a word
	if constexpr (CB == 8) {
		thr_word = threshold;
	} else {
		if (threshold > Swar<CB>::kOnes) // no counter reaches it: every vector counts as zero
			src_n_vec = 0;
		thr_word = (threshold > Swar<CB>::kOnes ? Swar<CB>::kOnes : threshold) * Swar<CB>::kLsb;
	}
	const uint64_t total = out_words * (64 / (16 / CB));
	uint64_t blocks = (total + 255) / 256;
	if (blocks > 4096)
		blocks = 4096;
	hipLaunchKernelGGL((threshold_kernel<CB>), dim3((unsigned)blocks), dim3(256), 0, s, src, src_n_vec, thr_word,
	                   static_cast<uint64_t*>(out), out_words);
	return hipGetLastError();
}

} // namespace

hipError_t launch_combine(int counter_bytes, int op, void* dst, const CombineSrcs& srcs, unsigned n, uint64_t nbytes,
                          unsigned long long* pop, hipStream_t s)
{
	if (nbytes % 16 || n == 0 || n > kCombineMaxSrcs)
		return hipErrorInvalidValue;
	const uint64_t n_vec = nbytes / 16;
	if (n_vec == 0)
		return hipSuccess;
	switch (counter_bytes) {
	case 0: return combine_cb<0>(op, dst, srcs, n, n_vec, pop, s);
	case 1: return combine_cb<1>(op, dst, srcs, n, n_vec, pop, s);
	case 2: return combine_cb<2>(op, dst, srcs, n, n_vec, pop, s);
	case 4: return combine_cb<4>(op, dst, srcs, n, n_vec, pop, s);
	case 8: return combine_cb<8>(op, dst, srcs, n, n_vec, pop, s);
	default: return hipErrorInvalidValue;
	}
}

hipError_t launch_fold(int counter_bytes, const void* src, uint64_t stride, uint64_t valid, uint64_t n_slices,
                       uint64_t per_group, uint64_t groups, void* dst, uint64_t row_bytes, hipStream_t s)
{
	if (row_bytes % 16 || row_bytes == 0 || valid == 0 || valid > row_bytes || n_slices == 0 || per_group == 0 ||
	    groups == 0 || groups > 65535 || (groups - 1) * per_group >= n_slices)
		return hipErrorInvalidValue;
	const uint64_t n_vec = row_bytes / 16;
	switch (counter_bytes) {
	case 0: return fold_cb<0>(src, stride, valid, n_slices, per_group, groups, dst, n_vec, s);
	case 1: return fold_cb<1>(src, stride, valid, n_slices, per_group, groups, dst, n_vec, s);
	case 2: return fold_cb<2>(src, stride, valid, n_slices, per_group, groups, dst, n_vec, s);
	case 4: return fold_cb<4>(src, stride, valid, n_slices, per_group, groups, dst, n_vec, s);
	case 8: return fold_cb<8>(src, stride, valid, n_slices, per_group, groups, dst, n_vec, s);
	default: return hipErrorInvalidValue;
	}
}

hipError_t launch_threshold_bits(int counter_bytes, const void* src, uint64_t src_bytes, uint64_t threshold, void* out,
                                 uint64_t out_words, hipStream_t s)
{
	if (src_bytes % 16 || threshold == 0)
		return hipErrorInvalidValue;
	if (out_words == 0)
		return hipSuccess;
	switch (counter_bytes) {
	case 1: return threshold_cb<1>(src, src_bytes / 16, threshold, out, out_words, s);
	case 2: return threshold_cb<2>(src, src_bytes / 16, threshold, out, out_words, s);
	case 4: return threshold_cb<4>(src, src_bytes / 16, threshold, out, out_words, s);
	case 8: return threshold_cb<8>(src, src_bytes / 16, threshold, out, out_words, s);
	default: return hipErrorInvalidValue;
	}
}

} // namespace btlbf
