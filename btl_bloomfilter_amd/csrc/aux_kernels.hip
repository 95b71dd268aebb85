// csrc/aux_kernels.hip -- everything around the fused sequence kernel:
//   * probes from precomputed hash rows (BloomFilter::insert/contains/insertAndCheck(const uint64_t[]),
//     BloomFilter.hpp:185-262; CountingBloomFilter minCount/insert/incrementAll, :53-64,135-183),
//     in parallel or in strict serial order (one lane) for order-dependent operations
//   * hash rows of raw k-mers (KmerBloomFilter::insert / contains(const char*))
//   * popcount reductions (getPop BloomFilter.hpp:316-323; popCount/filtered_popcount
//     CountingBloomFilter.hpp:217-242)
//   * the digest of an array and the comparison of two, computed where they lie (btlbf_digest, btlbf_compare)
//   * synthetic read generator and the random-access microbenchmarks
//   * shard-local position insert/test and the origin-side AND of routed answers
//   * per-sequence totals of a per-window bitmap (count_per_seq)
//   * the rank structure over a bit filter (miBF stage 2) and its queries
// (the split query's kernels are a unit of their own, split_query_kernels.hip)
#include "seq_core.hpp"

namespace btlbf {


template <bool POW2>
__device__ __forceinline__ void hash_row_op(int op, void* filter, const ModParams& mod, uint32_t h,
                                            uint32_t threshold, const uint64_t* row, uint8_t* out)
{
	uint32_t* words = static_cast<uint32_t*>(filter);
	switch (op) {
	case H_BF_INSERT:
		for (uint32_t i = 0; i < h; ++i) {
			const uint64_t p = reduce_mod<POW2>(row[i], mod) - mod.shard_lo;
			if (p < mod.shard_len)
				bf_set(words, p);
		}
		break;
	case H_BF_CONTAINS: {
		uint32_t all = 1;
		for (uint32_t i = 0; i < h; ++i) {
			const uint64_t p = reduce_mod<POW2>(row[i], mod);
			all &= (bf_word(words, p) >> (p & 31)) & 1u;
		}
		*out = (uint8_t)all;
		break;
	}
	case H_BF_INSERT_CHECK: {
		uint32_t all = 1;
		for (uint32_t i = 0; i < h; ++i)
			all &= bf_set_fetch(words, reduce_mod<POW2>(row[i], mod));
		*out = (uint8_t)all;
		break;
	}
	case H_CBF_INC_ALL:
		for (uint32_t i = 0; i < h; ++i)
			cbf_inc_sat(words, reduce_mod<POW2>(row[i], mod));
		break;
	case H_CBF_MIN:
	case H_CBF_CONTAINS:
	case H_CBF_INSERT_CHECK:
	case H_CBF_INC_MIN: {
		if (op != H_CBF_INC_MIN) {
			uint32_t mn = 0xffu;
			for (uint32_t i = 0; i < h; ++i) {
				const uint32_t v = cbf_read_fresh(words, reduce_mod<POW2>(row[i], mod));
				mn = v < mn ? v : mn;
			}
			*out = op == H_CBF_MIN ? (uint8_t)mn : (uint8_t)(mn >= threshold);
			if (op != H_CBF_INSERT_CHECK)
				break;
		}
		// incrementMin, CountingBloomFilter.hpp:135-162
		for (;;) {
			uint32_t mn = 0xffu;
			for (uint32_t i = 0; i < h; ++i) {
				const uint32_t v = cbf_read_fresh(words, reduce_mod<POW2>(row[i], mod));
				mn = v < mn ? v : mn;
			}
			if (mn == 0xffu)
				break;
			bool done = false;
			for (uint32_t i = 0; i < h; ++i)
				done |= cbf_cas_byte(words, reduce_mod<POW2>(row[i], mod), mn);
			if (done)
				break;
		}
		break;
	}
	default: break;
	}
}

// one lane per hash row; rows whose row_valid byte is 0 are skipped (out = 0)
template <bool POW2>
__global__ __launch_bounds__(256) void hash_rows_kernel(int op, void* filter, ModParams mod, uint32_t h,
                                                        uint32_t threshold, const uint64_t* hashes,
                                                        uint64_t n, const uint8_t* row_valid, uint8_t* out)
{
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
	     r += (uint64_t)gridDim.x * blockDim.x) {
		uint8_t o = 0;
		if (!row_valid || row_valid[r])
			hash_row_op<POW2>(op, filter, mod, h, threshold, hashes + r * h, &o);
		if (out)
			out[r] = o;
	}
}

// strict row order on one lane: the only reproducible form of the order-dependent operations
// (incrementMin, insertAndCheck on streams with repeats); valid_bits: one bit per row, row_valid: one byte
template <bool POW2>
__global__ void hash_rows_serial_kernel(int op, void* filter, ModParams mod, uint32_t h,
                                        uint32_t threshold, const uint64_t* hashes, uint64_t n,
                                        const uint8_t* valid_bits, const uint8_t* row_valid, uint8_t* out)
{
	if (blockIdx.x != 0 || threadIdx.x != 0)
		return;
	for (uint64_t r = 0; r < n; ++r) {
		if (valid_bits && !((valid_bits[r >> 3] >> (r & 7)) & 1))
			continue;
		uint8_t o = 0;
		if (!row_valid || row_valid[r])
			hash_row_op<POW2>(op, filter, mod, h, threshold, hashes + r * h, &o);
		if (out)
			out[r] = o;
	}
}

hipError_t launch_hash_op(int op, void* filter, const ModParams& mod, uint32_t h, uint32_t threshold,
                          const uint64_t* hashes, uint64_t n, uint8_t* out, int serial, hipStream_t s,
                          const uint8_t* row_valid)
{
	if (n == 0)
		return hipSuccess;
	if (serial) {
		if (mod.pow2)
			hipLaunchKernelGGL(hash_rows_serial_kernel<true>, dim3(1), dim3(64), 0, s, op, filter, mod, h,
			                   threshold, hashes, n, (const uint8_t*)nullptr, row_valid, out);
		else
			hipLaunchKernelGGL(hash_rows_serial_kernel<false>, dim3(1), dim3(64), 0, s, op, filter, mod, h,
			                   threshold, hashes, n, (const uint8_t*)nullptr, row_valid, out);
		return hipGetLastError();
	}
	uint64_t blocks = (n + 255) / 256;
	if (blocks > 2048)
		blocks = 2048;
	if (mod.pow2)
		hipLaunchKernelGGL(hash_rows_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, op, filter, mod,
		                   h, threshold, hashes, n, row_valid, out);
	else
		hipLaunchKernelGGL(hash_rows_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, op, filter, mod,
		                   h, threshold, hashes, n, row_valid, out);
	return hipGetLastError();
}

// ---- raw k-mers: KmerBloomFilter::insert / contains(const char*) (KmerBloomFilter.hpp:47-74) -----------
// The reference hashes a raw k-mer with NTC64(kmerSeq, k) (vendor/nthash.hpp:394-439,460-465): a walk through
// 4-/3-/2-mer tables indexed by convertTab / RCconvertTab codes -- a Horner chain over base codes, with
// rolx(h,4) + swapxbits033(h,4) = srol^4.  Its values differ from the iterator's (NTMC64) in the cases below, and
// this kernel returns what the reference's x86-64 build returns (tests/golden/hash_vectors.json "kmer"):
//   * U/u read as A (convertTab 0, RCconvertTab 3; nthash.hpp:16-86), except in a one-base remainder
//     (k % 4 == 1), which goes through seedTab and reads U as T (:416-417,432-433);
//   * k % 4 == 0: the forward walk ends with rolx(h, 0) and swapxbits033(h, 0); their shifts by 64 execute as
//     shifts by 0 on x86-64, so h becomes h ^ (y | y << 33) with y = h ^ (h >> 33) (:354-356,388-391,404-406);
//   * a byte that is not a base has code 255 and table indices / offsets are uint8_t: they wrap modulo 256;
//   * a 2- or 3-base remainder whose wrapped index lies beyond dimerTab[16] / trimerTab[64] reads outside the
//     reference's tables (undefined): the k-mer is reported invalid and skipped.
// One lane per k-mer; rows[r*h ..] = the h hash values (NTE64, :537-542), valid[r] = 0 for a skipped k-mer.
__device__ __forceinline__ uint32_t kmer_conv(uint32_t c, bool rc)
{
	switch (c) {
	case 'A': case 'a': case 'U': case 'u': return rc ? 3u : 0u;
	case 'C': case 'c': return rc ? 2u : 1u;
	case 'G': case 'g': return rc ? 1u : 2u;
	case 'T': case 't': return rc ? 0u : 3u;
	default: return 255u;
	}
}
__device__ __forceinline__ uint64_t kmer_seed(uint32_t d)
{
	return d == 0 ? kSeedA : d == 1 ? kSeedC : d == 2 ? kSeedG : kSeedT;
}
// seedTab (vendor/nthash.hpp:195-228), for the one-base remainder
__device__ __forceinline__ uint64_t kmer_seed_tab(uint32_t c)
{
	switch (c) {
	case 'A': case 'a': case 4: case 5: return kSeedA;
	case 'C': case 'c': case 7: return kSeedC;
	case 'G': case 'g': case 3: return kSeedG;
	case 'T': case 't': case 'U': case 'u': case 1: return kSeedT;
	default: return 0;
	}
}
// h <- srol^n(h) ^ table_n[idx]: n Horner steps over the base-4 digits of idx, most significant first
__device__ __forceinline__ uint64_t kmer_mer_step(uint64_t hv, uint32_t idx, int n)
{
	for (int j = n - 1; j >= 0; --j)
		hv = srol1(hv) ^ kmer_seed((idx >> (2 * j)) & 3u);
	return hv;
}

__global__ __launch_bounds__(256) void kmer_rows_kernel(const uint8_t* kmers, uint64_t n, uint32_t k, uint32_t h,
                                                        uint64_t kms, uint64_t* rows, uint8_t* valid)
{
	const uint32_t q = k / 4, r = k % 4;
	for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
	     row += (uint64_t)gridDim.x * blockDim.x) {
		const uint8_t* s = kmers + row * k;
		uint64_t f = 0, v = 0;
		bool ok = true;
		for (uint32_t i = 0; i < q; ++i) { // NTF64(kmerSeq, k), :394-407
			const uint32_t off = (4 * i) & 255u;
			const uint32_t loc = (64 * kmer_conv(s[off], false) + 16 * kmer_conv(s[off + 1], false) +
			                      4 * kmer_conv(s[off + 2], false) + kmer_conv(s[off + 3], false)) & 255u;
			f = kmer_mer_step(f, loc, 4);
		}
		if (r == 0) {
			const uint64_t y = f ^ (f >> 33);
			f ^= y | (y << 33);
		} else if (r == 1) {
			f = srol1(f) ^ kmer_seed_tab(s[k - 1]);
			v = kmer_seed_tab(s[k - 1] & 7u);
		} else {
			uint32_t lf = 0, lr = 0;
			for (uint32_t j = 0; j < r; ++j) {
				lf = 4 * lf + kmer_conv(s[k - r + j], false);
				lr = 4 * lr + kmer_conv(s[k - 1 - j], true);
			}
			lf &= 255u;
			lr &= 255u;
			ok = lf < (1u << (2 * r)) && lr < (1u << (2 * r));
			f = kmer_mer_step(f, lf, (int)r);
			v = kmer_mer_step(0, lr, (int)r);
		}
		for (uint32_t i = 0; i < q; ++i) { // NTR64(kmerSeq, k), :423-439
			const uint32_t off = (4 * (q - i) - 1) & 255u;
			const uint32_t loc = (64 * kmer_conv(s[off], true) + 16 * kmer_conv(s[off - 1], true) +
			                      4 * kmer_conv(s[off - 2], true) + kmer_conv(s[off - 3], true)) & 255u;
			v = kmer_mer_step(v, loc, 4);
		}
		const uint64_t b = v < f ? v : f; // NTC64, :460-465
		rows[row * h] = ok ? b : 0;
		for (uint32_t i = 1; i < h; ++i)
			rows[row * h + i] = ok ? extra_hash(b, kms, i) : 0;
		valid[row] = ok ? 1 : 0;
	}
}

hipError_t launch_kmer_rows(const uint8_t* kmers, uint64_t n, uint32_t k, uint32_t h, uint64_t kms, uint64_t* rows,
                            uint8_t* valid, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	uint64_t blocks = (n + 255) / 256;
	if (blocks > 4096)
		blocks = 4096;
	hipLaunchKernelGGL(kmer_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, kmers, n, k, h, kms, rows, valid);
	return hipGetLastError();
}

// serial-order update over the dense hash rows of a sequence buffer (row p = window p; rows of
// unclean windows are skipped through valid_bits).  op is a HashOp.
hipError_t launch_serial_seq_update(const SeqArgs& a, int op, const uint64_t* hashes,
                                    const uint8_t* valid_bits, uint8_t* out, hipStream_t s)
{
	if (a.len == 0)
		return hipSuccess;
	if (a.mod.pow2)
		hipLaunchKernelGGL(hash_rows_serial_kernel<true>, dim3(1), dim3(64), 0, s, op, a.filter, a.mod,
		                   a.hp.h, a.threshold, hashes, a.len, valid_bits, (const uint8_t*)nullptr, out);
	else
		hipLaunchKernelGGL(hash_rows_serial_kernel<false>, dim3(1), dim3(64), 0, s, op, a.filter, a.mod,
		                   a.hp.h, a.threshold, hashes, a.len, valid_bits, (const uint8_t*)nullptr, out);
	return hipGetLastError();
}

// ---- popcount ----------------------------------------------------------------------------------
// mode 0: set bits; mode 1: non-zero bytes; mode 2: bytes >= threshold.  nbytes must be a multiple
// of 8 (bitmaps are whole uint64_t words; filter arrays are zero-padded to 16 bytes).
__global__ __launch_bounds__(256) void popcount_kernel(const uint2* data, uint64_t n_vec, int mode,
                                                       uint32_t threshold, unsigned long long* out)
{
	unsigned long long acc = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec;
	     i += (uint64_t)gridDim.x * blockDim.x) {
		const uint2 v = data[i];
		const uint32_t w[2] = {v.x, v.y};
#pragma unroll
		for (int q = 0; q < 2; ++q) {
			if (mode == 0) {
				acc += __popc(w[q]);
			} else {
#pragma unroll
				for (int b = 0; b < 4; ++b) {
					const uint32_t c = (w[q] >> (8 * b)) & 0xff;
					acc += mode == 1 ? (c != 0) : (c >= threshold);
				}
			}
		}
	}
	// wave reduce, then one atomic per wave
	for (int o = 32; o > 0; o >>= 1)
		acc += __shfl_xor(acc, o, 64);
	if ((threadIdx.x & 63) == 0 && acc)
		atomicAdd(out, acc);
}

hipError_t launch_popcount(const void* data, uint64_t nbytes, int mode, uint32_t threshold,
                           unsigned long long* out, hipStream_t s)
{
	if (nbytes % 8)
		return hipErrorInvalidValue;
	const uint64_t n_vec = nbytes / 8;
	if (n_vec == 0)
		return hipSuccess;
	uint64_t blocks = (n_vec + 255) / 256;
	if (blocks > 4096)
		blocks = 4096;
	hipLaunchKernelGGL(popcount_kernel, dim3((unsigned)blocks), dim3(256), 0, s,
	                   static_cast<const uint2*>(data), n_vec, mode, threshold, out);
	return hipGetLastError();
}

// ---- digest of an array, computed where it lies (btlbf_digest) -------------------------------------------
// out[0] += sum of w_i * m_i (mod 2^64), out[1] ^= xor of mix64(w_i ^ m_i) over the non-zero 64-bit words w_i, where
// i = word0 + (index of the word in this array) is the word's index in the WHOLE filter and m_i = mix64(i + 1) | 1.
// Zero words contribute nothing, so the digests of shards combine (add / xor) to the digest of the whole filter
// whatever the split.  Streaming like popcount_kernel: 16-byte loads, one pair of atomics per wave.
__global__ __launch_bounds__(256) void digest_kernel(const uint4* data, uint64_t n_vec, uint64_t word0,
                                                     unsigned long long* out)
{
	unsigned long long sum = 0, x = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec;
	     i += (uint64_t)gridDim.x * blockDim.x) {
		typedef uint32_t v4u __attribute__((ext_vector_type(4)));
		const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(data) + i);
		const uint64_t w[2] = {((uint64_t)v.y << 32) | v.x, ((uint64_t)v.w << 32) | v.z};
#pragma unroll
		for (int q = 0; q < 2; ++q) {
			if (w[q]) {
				const uint64_t m = mix64(word0 + 2 * i + q + 1) | 1ull;
				sum += w[q] * m;
				x ^= mix64(w[q] ^ m);
			}
		}
	}
	for (int o = 32; o > 0; o >>= 1) {
		sum += __shfl_xor(sum, o, 64);
		x ^= __shfl_xor(x, o, 64);
	}
	if ((threadIdx.x & 63) == 0) {
		if (sum)
			atomicAdd(out, sum);
		if (x)
			atomicXor(out + 1, x);
	}
}

hipError_t launch_digest(const void* data, uint64_t nbytes, uint64_t word0, unsigned long long* out2, hipStream_t s)
{
	if (nbytes % 16)
		return hipErrorInvalidValue;
	const uint64_t n_vec = nbytes / 16;
	if (n_vec == 0)
		return hipSuccess;
	uint64_t blocks = (n_vec + 255) / 256;
	if (blocks > 8192)
		blocks = 8192;
	hipLaunchKernelGGL(digest_kernel, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint4*>(data), n_vec,
	                   word0, out2);
	return hipGetLastError();
}

// ---- compare two arrays of the same geometry (btlbf_compare) ---------------------------------------
// counting == 0: positions are bits; out[0] += bits that differ, out[1] += bits set only in a, out[2] += bits
// set only in b.  counting != 0: positions are uint8_t counters; out[0] += counters that differ, out[1] +=
// counters with a > b, out[2] += counters with a < b.
__global__ __launch_bounds__(256) void compare_kernel(const uint2* a, const uint2* b, uint64_t n_vec, int counting,
                                                      unsigned long long* out)
{
	unsigned long long gt = 0, lt = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec;
	     i += (uint64_t)gridDim.x * blockDim.x) {
		const uint2 va = a[i], vb = b[i];
		const uint32_t wa[2] = {va.x, va.y}, wb[2] = {vb.x, vb.y};
#pragma unroll
		for (int q = 0; q < 2; ++q) {
			if (!counting) {
				gt += __popc(wa[q] & ~wb[q]);
				lt += __popc(wb[q] & ~wa[q]);
			} else if (wa[q] != wb[q]) {
#pragma unroll
				for (int c = 0; c < 4; ++c) {
					const uint32_t ca = (wa[q] >> (8 * c)) & 0xff, cb = (wb[q] >> (8 * c)) & 0xff;
					gt += ca > cb;
					lt += ca < cb;
				}
			}
		}
	}
	for (int o = 32; o > 0; o >>= 1) {
		gt += __shfl_xor(gt, o, 64);
		lt += __shfl_xor(lt, o, 64);
	}
	if ((threadIdx.x & 63) == 0 && (gt | lt)) {
		atomicAdd(out, gt + lt);
		atomicAdd(out + 1, gt);
		atomicAdd(out + 2, lt);
	}
}

hipError_t launch_compare(const void* a, const void* b, uint64_t nbytes, int counting, unsigned long long* out3,
                          hipStream_t s)
{
	if (nbytes % 8)
		return hipErrorInvalidValue;
	const uint64_t n_vec = nbytes / 8;
	if (n_vec == 0)
		return hipSuccess;
	uint64_t blocks = (n_vec + 255) / 256;
	if (blocks > 4096)
		blocks = 4096;
	hipLaunchKernelGGL(compare_kernel, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint2*>(a),
	                   static_cast<const uint2*>(b), n_vec, counting, out3);
	return hipGetLastError();
}

// ---- synthetic reads --------------------------------------------------------------
// read r, base j = "ACGT"[(w(r*wpr + j/32) >> 2*(j%32)) & 3], w(n) = mix64(seed + (n+1)*golden)
__global__ __launch_bounds__(256) void synth_kernel(uint8_t* out, uint64_t seed, uint64_t first,
                                                    uint64_t total_bytes, uint32_t read_len)
{
	const uint32_t wpr = (read_len + 31) / 32;
	for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c * 16 < total_bytes;
	     c += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t o = c * 16;
		uint64_t r = o / read_len;
		uint32_t j = (uint32_t)(o - r * read_len);
		uint64_t cur_n = ~0ull, w = 0;
		uint32_t ow[4] = {0, 0, 0, 0};
		for (int b = 0; b < 16; ++b) {
			if (o + b >= total_bytes)
				break;
			const uint64_t n = (first + r) * wpr + (j >> 5);
			if (n != cur_n) {
				cur_n = n;
				w = mix64(seed + (n + 1) * 0x9E3779B97F4A7C15ULL);
			}
			const uint32_t code = (uint32_t)(w >> (2 * (j & 31))) & 3;
			const uint32_t ch = (0x54474341u >> (8 * code)) & 0xff; // "ACGT"
			ow[b >> 2] |= ch << (8 * (b & 3));
			if (++j == read_len) {
				j = 0;
				++r;
			}
		}
		if (o + 16 <= total_bytes) {
			*reinterpret_cast<uint4*>(out + o) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
		} else {
			for (int b = 0; o + b < total_bytes; ++b)
				out[o + b] = (uint8_t)(ow[b >> 2] >> (8 * (b & 3)));
		}
	}
}

hipError_t launch_synth(uint8_t* out, uint64_t seed, uint64_t first, uint64_t n, uint32_t read_len,
                        hipStream_t s)
{
	const uint64_t total = n * read_len;
	if (total == 0)
		return hipSuccess;
	uint64_t blocks = ((total + 15) / 16 + 255) / 256;
	if (blocks > 8192)
		blocks = 8192;
	hipLaunchKernelGGL(synth_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, seed, first, total,
	                   read_len);
	return hipGetLastError();
}

// ---- random-access microbenchmarks ---------------------------------------------------------------
// kind 0: 4-byte loads, kind 1: 4-byte atomicOr; uniformly random 64-byte-aligned offsets; 8
// independent accesses per lane per round so the memory system, not latency, is the limit.
__global__ __launch_bounds__(256) void microbench_kernel(uint32_t* data, uint64_t n_lines, int kind,
                                                         uint64_t rounds, unsigned long long* sink)
{
	const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
	uint32_t acc = 0;
	for (uint64_t it = 0; it < rounds; ++it) {
		uint64_t idx[8];
#pragma unroll
		for (int u = 0; u < 8; ++u) {
			const uint64_t x = mix64((it * 8 + u) * nthreads + gid + 0x1234567ull);
			idx[u] = (__umul64hi(x, n_lines)) * 16; // uint32 index of a 64-byte line start
		}
		if (kind == 0) {
#pragma unroll
			for (int u = 0; u < 8; ++u)
				acc ^= data[idx[u]];
		} else {
#pragma unroll
			for (int u = 0; u < 8; ++u)
				atomicOr(data + idx[u], 1u << (idx[u] >> 4 & 31));
		}
	}
	if (kind == 0 && acc == 0x9e3779b9u)
		atomicAdd(sink, 1ull); // keeps the loads alive
}

hipError_t launch_microbench(void* data, uint64_t nbytes, int kind, uint64_t n_access,
                             unsigned long long* sink, hipStream_t s)
{
	const uint64_t n_lines = nbytes / 64;
	if (n_lines == 0)
		return hipErrorInvalidValue;
	const unsigned blocks = 256 * 8;
	const uint64_t nthreads = (uint64_t)blocks * 256;
	uint64_t rounds = n_access / (nthreads * 8);
	if (rounds == 0)
		rounds = 1;
	hipLaunchKernelGGL(microbench_kernel, dim3(blocks), dim3(256), 0, s, static_cast<uint32_t*>(data),
	                   n_lines, kind, rounds, sink);
	return hipGetLastError();
}

// ---- shard-local positions (multi-GPU) -------------------------------------------------------------
__global__ __launch_bounds__(256) void positions_kernel(int test, uint32_t* words, int counting,
                                                        const uint64_t* pos, uint64_t n, uint8_t* out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
	     i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t p = pos[i];
		if (!test)
			bf_set(words, p);
		else
			out[i] = (uint8_t)((bf_word(words, p) >> (p & 31)) & 1u);
	}
	(void)counting;
}

hipError_t launch_positions(int test, void* filter, const ModParams& mod, const uint64_t* pos,
                            uint64_t n, uint8_t* out, hipStream_t s)
{
	(void)mod;
	if (n == 0)
		return hipSuccess;
	uint64_t blocks = (n + 255) / 256;
	if (blocks > 2048)
		blocks = 2048;
	hipLaunchKernelGGL(positions_kernel, dim3((unsigned)blocks), dim3(256), 0, s, test,
	                   static_cast<uint32_t*>(filter), 0, pos, n, out);
	return hipGetLastError();
}

// origin side of a sharded query: a probe that missed clears its window's bit
__global__ __launch_bounds__(256) void and_answers_kernel(const uint64_t* tags, const uint8_t* answers,
                                                          uint64_t n, uint32_t h, uint64_t* hit_bits)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
	     i += (uint64_t)gridDim.x * blockDim.x) {
		if (!answers[i]) {
			const uint64_t p = tags[i] / h;
			atomicAnd(reinterpret_cast<unsigned long long*>(hit_bits) + (p >> 6),
			          ~(1ull << (p & 63)));
		}
	}
}

hipError_t launch_and_answers(const uint64_t* tags, const uint8_t* answers, uint64_t n, uint32_t h,
                              uint64_t* hit_bits, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	uint64_t blocks = (n + 255) / 256;
	if (blocks > 2048)
		blocks = 2048;
	hipLaunchKernelGGL(and_answers_kernel, dim3((unsigned)blocks), dim3(256), 0, s, tags, answers, n, h,
	                   hit_bits);
	return hipGetLastError();
}

// ---- per-sequence totals of a per-window bitmap (what read classifiers consume) --------------------
// set bits of `bits` in window range [lo, hi) (bit p of the bitmap = window starting at byte p)
__device__ __forceinline__ uint32_t popc_range(const uint64_t* bits, uint64_t lo, uint64_t hi)
{
	if (hi <= lo)
		return 0;
	uint32_t n = 0;
	const uint64_t w0 = lo >> 6, w1 = (hi - 1) >> 6;
	for (uint64_t w = w0; w <= w1; ++w) {
		uint64_t x = bits[w];
		if (w == w0)
			x &= ~0ull << (lo & 63);
		if (w == w1 && ((hi & 63) != 0))
			x &= ~0ull >> (64 - (hi & 63));
		n += __popcll(x);
	}
	return n;
}

__global__ __launch_bounds__(256) void count_per_seq_kernel(const uint64_t* hit_bits, const uint64_t* valid_bits,
                                                            uint64_t len, const uint64_t* starts, uint64_t n_seqs,
                                                            uint32_t read_len, uint32_t k, uint32_t* hits_out,
                                                            uint32_t* valid_out)
{
	for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_seqs;
	     s += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t b = starts ? starts[s] : s * read_len;
		uint64_t e = starts ? starts[s + 1] : b + read_len;
		if (e > len)
			e = len;
		const uint64_t hi = e >= b + k ? e - k + 1 : b; // windows of this sequence start in [b, hi)
		hits_out[s] = popc_range(hit_bits, b, hi);
		if (valid_out)
			valid_out[s] = valid_bits ? popc_range(valid_bits, b, hi) : (uint32_t)(hi - b);
	}
}

hipError_t launch_count_per_seq(const uint64_t* hit_bits, const uint64_t* valid_bits, uint64_t len,
                                const uint64_t* starts, uint64_t n_seqs, uint32_t read_len, uint32_t k,
                                uint32_t* hits_out, uint32_t* valid_out, hipStream_t s)
{
	if (n_seqs == 0)
		return hipSuccess;
	uint64_t blocks = (n_seqs + 255) / 256;
	if (blocks > 65536)
		blocks = 65536;
	hipLaunchKernelGGL(count_per_seq_kernel, dim3((unsigned)blocks), dim3(256), 0, s, hit_bits, valid_bits, len, starts,
	                   n_seqs, read_len, k, hits_out, valid_out);
	return hipGetLastError();
}

// ---- rank structure over a bit filter (miBF stage 2: sdsl::bit_vector_il<512> + rank_support_il<1>) --------
// The reference's multi-index Bloom filter turns a set bit's position into an index of its ID array with
// rank(pos) = number of set bits before pos (MIBloomFilter.hpp:527 getRankPos, :324,391,443,461,488,509,522),
// over sdsl's INTERLEAVED bit vector (MIBloomFilter.hpp:44,133,144,801-803): the bit vector cut into blocks of
// 512 bits, each preceded by one 64-bit word holding the number of set bits before the block, so that one
// rank query touches one 72-byte record.  sdsl-lite is not vendored with the reference (SURVEY.md section 2,
// row 9); this is its published layout: record b = { ones before bit 512*b, data words 8*b .. 8*b+7 }.
static constexpr uint32_t kRankBlockWords = 8; // 512 bits

// pass 1: ones per 512-bit block.  pass 3 (after the scan of `ones`): write the interleaved records.
__global__ __launch_bounds__(256) void rank_block_ones_kernel(const uint64_t* bits, uint64_t n_words, uint64_t n_blocks,
                                                              uint64_t* ones)
{
	for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t c = 0;
#pragma unroll
		for (uint32_t j = 0; j < kRankBlockWords; ++j) {
			const uint64_t w = b * kRankBlockWords + j;
			c += w < n_words ? (uint32_t)__popcll(bits[w]) : 0;
		}
		ones[b] = c;
	}
}

// exclusive prefix sum of n values in place, by ONE workgroup: every thread owns a contiguous slice
__global__ __launch_bounds__(1024) void scan_u64_kernel(uint64_t* v, uint64_t n, uint64_t* total)
{
	__shared__ uint64_t part[1024];
	const uint64_t per = (n + 1023) / 1024;
	const uint64_t lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
	uint64_t sum = 0;
	for (uint64_t i = lo; i < hi; ++i)
		sum += v[i];
	part[threadIdx.x] = sum;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t run = 0;
		for (int t = 0; t < 1024; ++t) {
			const uint64_t x = part[t];
			part[t] = run;
			run += x;
		}
		if (total)
			*total = run;
	}
	__syncthreads();
	uint64_t run = part[threadIdx.x];
	for (uint64_t i = lo; i < hi; ++i) {
		const uint64_t x = v[i];
		v[i] = run;
		run += x;
	}
}

// two-level: chunk sums (4096 blocks a chunk) -> scan of the chunk sums -> per-chunk exclusive scan
__global__ __launch_bounds__(256) void rank_chunk_sum_kernel(const uint64_t* ones, uint64_t n_blocks, uint64_t* chunk)
{
	__shared__ unsigned long long acc;
	if (threadIdx.x == 0)
		acc = 0;
	__syncthreads();
	unsigned long long c = 0;
	for (uint32_t j = threadIdx.x; j < 4096; j += 256) {
		const uint64_t b = (uint64_t)blockIdx.x * 4096 + j;
		c += b < n_blocks ? ones[b] : 0;
	}
	for (int o = 32; o > 0; o >>= 1)
		c += __shfl_xor(c, o, 64);
	if ((threadIdx.x & 63) == 0)
		atomicAdd(&acc, c);
	__syncthreads();
	if (threadIdx.x == 0)
		chunk[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void rank_write_kernel(const uint64_t* bits, uint64_t n_words, uint64_t n_blocks,
                                                         const uint64_t* ones, const uint64_t* chunk_base, uint64_t* il)
{
	// one workgroup per chunk of 4096 blocks; thread t scans blocks [16t, 16t+16) after a workgroup scan
	__shared__ uint64_t part[256];
	const uint64_t b0 = (uint64_t)blockIdx.x * 4096 + threadIdx.x * 16;
	uint64_t mine[16], sum = 0;
#pragma unroll
	for (int j = 0; j < 16; ++j) {
		mine[j] = b0 + j < n_blocks ? ones[b0 + j] : 0;
		sum += mine[j];
	}
	part[threadIdx.x] = sum;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t run = chunk_base[blockIdx.x];
		for (int t = 0; t < 256; ++t) {
			const uint64_t x = part[t];
			part[t] = run;
			run += x;
		}
	}
	__syncthreads();
	uint64_t run = part[threadIdx.x];
	for (int j = 0; j < 16; ++j) {
		const uint64_t b = b0 + j;
		if (b >= n_blocks)
			break;
		uint64_t* rec = il + b * (kRankBlockWords + 1);
		rec[0] = run;
		for (uint32_t q = 0; q < kRankBlockWords; ++q) {
			const uint64_t w = b * kRankBlockWords + q;
			rec[1 + q] = w < n_words ? bits[w] : 0;
		}
		run += mine[j];
	}
}

// rank_out[i] = set bits before position pos(i); bit_out[i] = the bit itself.  pos(i) = in[i] % size when `size`
// is given (in = hash values: getRankPos, MIBloomFilter.hpp:527), else in[i]
__global__ __launch_bounds__(256) void rank_query_kernel(const uint64_t* il, uint64_t n_bits, const uint64_t* in, uint64_t n,
                                                         const ModParams mod, int reduce, uint64_t* rank_out,
                                                         uint8_t* bit_out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t p = in[i];
		if (reduce)
			p = mod.pow2 ? (p & mod.mask) : reduce_mod<false>(p, mod);
		uint64_t r = 0;
		uint32_t bit = 0;
		if (p < n_bits) {
			const uint64_t* rec = il + (p >> 9) * (kRankBlockWords + 1);
			const uint32_t wq = (uint32_t)(p >> 6) & 7, sh = (uint32_t)p & 63;
			r = rec[0];
			for (uint32_t q = 0; q < wq; ++q)
				r += __popcll(rec[1 + q]);
			const uint64_t w = rec[1 + wq];
			r += __popcll(w & ((1ull << sh) - 1));
			bit = (uint32_t)(w >> sh) & 1u;
		}
		if (rank_out)
			rank_out[i] = r;
		if (bit_out)
			bit_out[i] = (uint8_t)bit;
	}
}

// scratch: n_blocks + ceil(n_blocks / 4096) + 1 uint64_t
hipError_t launch_rank_build(const uint64_t* bits, uint64_t n_bits, uint64_t* il, uint64_t* scratch, uint64_t* total_dev,
                             hipStream_t s)
{
	const uint64_t n_words = (n_bits + 63) / 64, n_blocks = (n_bits + 511) / 512;
	if (n_blocks == 0)
		return hipSuccess;
	const uint64_t n_chunks = (n_blocks + 4095) / 4096;
	if (n_chunks > (1ull << 31))
		return hipErrorInvalidValue;
	uint64_t* ones = scratch;
	uint64_t* chunk = scratch + n_blocks;
	uint64_t g = (n_blocks + 255) / 256;
	if (g > 65536)
		g = 65536;
	hipLaunchKernelGGL(rank_block_ones_kernel, dim3((unsigned)g), dim3(256), 0, s, bits, n_words, n_blocks, ones);
	hipLaunchKernelGGL(rank_chunk_sum_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, ones, n_blocks, chunk);
	hipLaunchKernelGGL(scan_u64_kernel, dim3(1), dim3(1024), 0, s, chunk, n_chunks, total_dev);
	hipLaunchKernelGGL(rank_write_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, bits, n_words, n_blocks, ones, chunk, il);
	return hipGetLastError();
}

hipError_t launch_rank_query(const uint64_t* il, uint64_t n_bits, const uint64_t* in, uint64_t n, const ModParams& mod,
                             int reduce, uint64_t* rank_out, uint8_t* bit_out, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	uint64_t g = (n + 255) / 256;
	if (g > 65536)
		g = 65536;
	hipLaunchKernelGGL(rank_query_kernel, dim3((unsigned)g), dim3(256), 0, s, il, n_bits, in, n, mod, reduce, rank_out, bit_out);
	return hipGetLastError();
}

} // namespace btlbf
