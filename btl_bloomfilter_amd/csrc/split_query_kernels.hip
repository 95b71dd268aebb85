// csrc/split_query_kernels.hip -- the kernels of the split query (host_query.cpp's SplitCold and SplitWarm routes):
//   * read_sample_kernel: the sampler that flags a read cold or warm (one lane per sampled read)
//   * the prefix sums over the flag words (cold-read ranks)
//   * compact_reads (warm and cold buffer) and gather_cold_reads (the cold reads and their index)
//   * the two merges of the compacted bitmaps back into the caller's layout
// and their launchers (declared in internal.hpp).
#include "seq_core.hpp"

namespace btlbf {

// ---- split query (fixed-length reads): likely-present and likely-absent reads take different paths ----
// contains() over a buffer whose misses come clustered by read (reads foreign to the indexed genome next to
// reads from it -- what a classifier feeds a filter): the partitioned path is fast when nearly every k-mer
// hits, the early-exit gather kernel when nearly none does.  So every read is SAMPLED (three of its windows,
// full contains() each), reads whose clean samples all miss are "cold", the buffer is compacted into a warm
// and a cold buffer, each goes down its own path, and the two bitmaps are merged back into the caller's
// layout.  Every path computes the exact contains(), so the sampling only steers speed.

// one lane per sampled read (read i * stride).  A read is COLD when most of its clean samples miss (two of
// three: a single false positive or a single SNP does not flip the call).  stride == 1: flags bit (r & 63) of
// word r >> 6 = read r is cold.  *n_cold += cold reads among the sampled ones.
// STAGED (stride == 1, 256 reads fit the LDS): the workgroup first copies its 256 consecutive reads into LDS with
// coalesced 16-byte loads and the lanes take their windows from there.  Straight from global memory every 4-byte
// load of a wave touches 64 different lines (one per read), more lines than the L1 holds between a lane's loads:
// the kernel spent as long on fetching 62 bytes per read as on its 8 probes per read.
template <bool STAGED>
__global__ __launch_bounds__(256) void read_sample_kernel(const uint8_t* seq, uint64_t n_reads, uint32_t L, uint32_t stride,
                                                          const HashParams hp, const ModParams mod, const void* filter,
                                                          uint32_t counting, uint32_t threshold, uint32_t probes2,
                                                          unsigned long long* flags, unsigned long long* n_cold)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t staged[]; // STAGED: 256 * L + 32 bytes
	__shared__ uint64_t tab[kNumCodes][2]; // Horner start-up seeds per base code (HashParams::init_tab)
	__shared__ uint8_t lut[256];           // byte -> code << 4 | flags (base_entry)
	if (threadIdx.x < kNumCodes * 2)
		tab[threadIdx.x >> 1][threadIdx.x & 1] = hp.init_tab[threadIdx.x >> 1][threadIdx.x & 1];
	lut[threadIdx.x] = base_entry(threadIdx.x); // 256 threads
	uint32_t staged_off = 0; // LDS byte offset of this lane's read
	if (STAGED) {
		const uint64_t r_wg = (uint64_t)blockIdx.x * 256;
		const uint64_t n_here = n_reads - r_wg < 256 ? n_reads - r_wg : 256; // (the grid covers n_reads exactly)
		const uintptr_t a0 = reinterpret_cast<uintptr_t>(seq) + r_wg * L;
		const uint32_t mis = (uint32_t)(a0 & 15);
		const uint32_t pieces = (uint32_t)((mis + n_here * L + 15) / 16);
		// (an aligned 16-byte piece that holds at least one byte of the buffer lies inside the buffer's last page)
		const uint4* src = reinterpret_cast<const uint4*>(a0 - mis);
		for (uint32_t p = threadIdx.x; p < pieces; p += 256)
			reinterpret_cast<uint4*>(staged)[p] = src[p];
		staged_off = mis + threadIdx.x * L;
	}
	__syncthreads();
	const uint64_t i_s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	// stride > 1: a pseudo-random read of every block of `stride` reads, so that input with a period (every
	// other read foreign, say) is not sampled in step with it
	const uint64_t r = i_s * stride + (stride > 1 ? mix64(i_s) % stride : 0);
	const uint32_t k = hp.k, W = L - k + 1;
	bool cold = false;
	if (r < n_reads) {
		const uint8_t* rd = seq + r * L;
		// one sample = full contains() of the window at `off`.  The hashing and the probing are separate steps so
		// that the probes of the first TWO samples -- 2h independent loads -- are requested together: one memory
		// latency for both (with one sample after the other the kernel ran at half the gather rate of the chip).
		// four bases of the read at byte offset o (STAGED: two aligned LDS words and a byte align)
		auto load4 = [&](uint32_t o) -> uint32_t {
			uint32_t word;
			if (STAGED) {
				const uint32_t a = staged_off + o;
				const uint32_t* l32 = reinterpret_cast<const uint32_t*>(staged) + (a >> 2);
				word = __builtin_amdgcn_alignbyte(l32[1], l32[0], a & 3);
			} else {
				__builtin_memcpy(&word, rd + o, 4);
			}
			return word;
		};
		auto hash_at = [&](uint32_t off, uint64_t& b) -> bool { // -> clean window; b = canonical base hash
			uint64_t fh = 0, rh = 0;
			uint32_t ok = kBaseValid;
			uint32_t i = 0;
			for (; i + 4 <= k; i += 4) { // four bases per (unaligned) load
				const uint32_t word = load4(off + i);
				// ACGT/acgt in one step (the byte permute of seq_stage_convert), anything else through the LUT
				const uint32_t idx = (word >> 1) & 0x03030303u;
				uint32_t e4;
				if ((word & 0xdfdfdfdfu) == __builtin_amdgcn_perm(0u, 0x47544341u, idx))
					e4 = __builtin_amdgcn_perm(0u, 0x23331303u, idx);
				else
					e4 = (uint32_t)lut[word & 0xff] | ((uint32_t)lut[(word >> 8) & 0xff] << 8) |
					     ((uint32_t)lut[(word >> 16) & 0xff] << 16) | ((uint32_t)lut[word >> 24] << 24);
#pragma unroll
				for (int b4 = 0; b4 < 4; ++b4) {
					const uint32_t e = (e4 >> (8 * b4)) & 0xff;
					ok &= e;
					fh = srol1(fh) ^ tab[e >> kCodeShift][0];
					rh = sror1(rh) ^ tab[e >> kCodeShift][1];
				}
			}
			for (; i < k; ++i) {
				const uint32_t e = lut[STAGED ? staged[staged_off + off + i] : rd[off + i]];
				ok &= e;
				fh = srol1(fh) ^ tab[e >> kCodeShift][0];
				rh = sror1(rh) ^ tab[e >> kCodeShift][1];
			}
			b = rh < fh ? rh : fh;
			return (ok & kBaseValid) != 0;
		};
		// what the filter holds at probe j of base hash b (bit filters: the bit; counting: the counter); unclean
		// windows probe position 0 (harmless) so that the loads stay unconditional
		auto fetch = [&](uint64_t b, uint32_t j) -> uint32_t {
			const uint64_t hv = j ? extra_hash(b, hp.kms, j) : b;
			const uint64_t p = mod.pow2 ? (hv & mod.mask) : reduce_mod<false>(hv, mod);
			if (counting)
				return cbf_read_fresh(static_cast<const uint32_t*>(filter), p);
			return (bf_word(static_cast<const uint32_t*>(filter), p) >> (p & 31)) & 1u;
		};
		auto all_hit = [&](uint64_t b) -> bool {
			bool hit = true;
			for (uint32_t j = 0; j < hp.h; ++j)
				hit &= counting ? fetch(b, j) >= threshold : fetch(b, j) != 0;
			return hit;
		};
		// The majority rule matters for the WARM side: a foreign read that slipped into the warm buffer on one
		// false-positive sample would put failures into the partitioned query and cost it a resolve pass over
		// everything; two false positives in one read do not happen.  The third sample is only looked at when the
		// first two disagree (or one of them was unclean).
		uint64_t b0 = 0, b1 = 0;
		const bool c0 = hash_at(0, b0);
		const bool c1 = W / 2 != 0 ? hash_at(W / 2, b1) : false;
		bool h0 = true, h1 = true;
		// (probes2 <= h probes of the second sample: what a present read costs is its probes -- all of them hit, so all
		// of them are loaded --, and the second sample is only there so that a foreign read does not pass on one
		// false-positive window; how many probes that takes depends on how many foreign reads there are: the caller
		// works it out from its estimate)
		for (uint32_t j = 0; j < hp.h; ++j) { // both samples' probes, interleaved: up to 2h loads before the first use
			const uint32_t v0 = fetch(c0 ? b0 : 0, j);
			h0 &= counting ? v0 >= threshold : v0 != 0;
			if (j < probes2) {
				const uint32_t v1 = fetch(c1 ? b1 : 0, j);
				h1 &= counting ? v1 >= threshold : v1 != 0;
			}
		}
		const uint32_t s0 = c0 ? (h0 ? 2u : 1u) : 0u, s1 = c1 ? (h1 ? 2u : 1u) : 0u; // 0 = unclean, 1 = miss, 2 = hit
		uint32_t clean = (s0 != 0) + (s1 != 0), misses = (s0 == 1) + (s1 == 1);
		if (!(s0 == s1 && s0 != 0) && W - 1 != W / 2) {
			uint64_t b2 = 0;
			const bool c2 = hash_at(W - 1, b2);
			const uint32_t s2 = c2 ? (all_hit(b2) ? 2u : 1u) : 0u;
			clean += s2 != 0;
			misses += s2 == 1;
		}
		cold = clean > 0 && 2 * misses > clean;
	}
	const unsigned long long m = __ballot(cold);
	if ((threadIdx.x & 63) == 0) {
		if (stride == 1 && r < n_reads)
			flags[r >> 6] = m;
		if (m)
			atomicAdd(n_cold, (unsigned long long)__popcll(m));
	}
}

// prefix[w] = cold reads before flag word w.  Three tiny passes: per-chunk sums (1024 words a chunk), a serial
// exclusive scan of the chunk sums by one thread (at most ~16 K chunks for 10^9 reads), then each word's
// prefix from its chunk's base
__global__ __launch_bounds__(1024) void flag_chunk_sum_kernel(const unsigned long long* flags, uint64_t n_words,
                                                             uint32_t* chunk_sum)
{
	__shared__ uint32_t acc;
	if (threadIdx.x == 0)
		acc = 0;
	__syncthreads();
	const uint64_t w = (uint64_t)blockIdx.x * 1024 + threadIdx.x;
	uint32_t c = w < n_words ? (uint32_t)__popcll(flags[w]) : 0;
	c = wave_sum(c);
	if ((threadIdx.x & 63) == 0 && c)
		atomicAdd(&acc, c);
	__syncthreads();
	if (threadIdx.x == 0)
		chunk_sum[blockIdx.x] = acc;
}
__global__ void flag_chunk_scan_kernel(uint32_t* chunk_sum, uint32_t n_chunks)
{
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		uint32_t run = 0;
		for (uint32_t i = 0; i < n_chunks; ++i) {
			const uint32_t v = chunk_sum[i];
			chunk_sum[i] = run;
			run += v;
		}
	}
}
__global__ __launch_bounds__(1024) void flag_prefix_kernel(const unsigned long long* flags, uint64_t n_words,
                                                          const uint32_t* chunk_base, uint32_t* prefix)
{
	__shared__ uint32_t wave_tot[16];
	const uint64_t w = (uint64_t)blockIdx.x * 1024 + threadIdx.x;
	const uint32_t c = w < n_words ? (uint32_t)__popcll(flags[w]) : 0;
	const uint32_t incl = wave_scan_incl(c);
	if ((threadIdx.x & 63) == 63)
		wave_tot[threadIdx.x >> 6] = incl;
	__syncthreads();
	uint32_t base = chunk_base[blockIdx.x];
	for (uint32_t v = 0; v < (threadIdx.x >> 6); ++v)
		base += wave_tot[v];
	if (w < n_words)
		prefix[w] = base + incl - c;
}

__device__ __forceinline__ uint32_t cold_rank(const unsigned long long* flags, const uint32_t* prefix, uint64_t r,
                                              bool* cold)
{
	const unsigned long long m = flags[r >> 6];
	*cold = (m >> (r & 63)) & 1ull;
	return prefix[r >> 6] + (uint32_t)__popcll(m & ((1ull << (r & 63)) - 1));
}

// One thread per 16-byte piece of a READ (ceil(L / 16) pieces per read, the last one short when L is no multiple of
// 16): consecutive lanes copy consecutive pieces of a read to cold_buf[rank * L + ...] or warm_buf[(r - rank) * L + ...],
// so that the loads and the stores of a wave are runs of (unaligned) 16-byte accesses, no piece straddles two reads
// and only the tail of a read is copied in smaller steps.  Measured on one box, 10^8 reads of 150 bytes, 1 % cold:
// 16-byte pieces of the SOURCE (a tenth of them straddle a read boundary and go byte by byte, and their whole wave
// with them) 20.4 ms; 4-byte pieces of a read 17.5 ms; the same with four pieces per thread in flight 23.8 ms.
__global__ __launch_bounds__(256) void compact_reads_kernel(const uint8_t* seq, uint64_t n_reads, uint32_t L, uint32_t ppr,
                                                            uint32_t ppr_inv, const unsigned long long* flags,
                                                            const uint32_t* prefix, uint8_t* warm_buf, uint8_t* cold_buf)
{
	// this workgroup's reads: 256 threads take 256 / ppr whole reads per trip (reads of more than 4096 bytes: one read
	// per trip, the threads loop over its pieces)
	const bool wide = ppr > 256;
	const uint32_t rpt = wide ? 1u : 256u / ppr; // reads per trip
	const uint32_t lr = wide ? 0u : __umulhi(threadIdx.x, ppr_inv), i0 = threadIdx.x - lr * ppr; // read of the trip, piece in it
	for (uint64_t r0 = (uint64_t)blockIdx.x * rpt; r0 < n_reads; r0 += (uint64_t)gridDim.x * rpt) {
		const uint64_t r = r0 + lr;
		if (lr >= rpt || r >= n_reads)
			continue;
		bool cold;
		const uint32_t rk = cold_rank(flags, prefix, r, &cold);
		const uint8_t* src0 = seq + r * L;
		uint8_t* dst0 = cold ? cold_buf + (uint64_t)rk * L : warm_buf + (r - rk) * L;
		for (uint32_t i = i0; i < ppr; i += wide ? 256u : ppr) {
			const uint8_t* src = src0 + 16 * i;
			uint8_t* dst = dst0 + 16 * i;
			if (16 * i + 16 <= L) {
				uint32_t w[4];
				__builtin_memcpy(w, src, 16); // unaligned loads / stores
				__builtin_memcpy(dst, w, 16);
			} else {
				const uint32_t n = L - 16 * i;
				uint32_t j = 0;
				for (; j + 4 <= n; j += 4) {
					uint32_t w;
					__builtin_memcpy(&w, src + j, 4);
					__builtin_memcpy(dst + j, &w, 4);
				}
				for (; j < n; ++j)
					dst[j] = src[j];
			}
		}
	}
}

// bits [pos, pos + n) of a bitmap (n <= 64), little-endian bit order
__device__ __forceinline__ uint64_t bits_at(const uint64_t* bm, uint64_t pos, uint32_t n)
{
	const uint64_t w = pos >> 6;
	const uint32_t sh = (uint32_t)(pos & 63);
	uint64_t v = bm[w] >> sh;
	if (sh + n > 64)
		v |= bm[w + 1] << (64 - sh);
	return n == 64 ? v : v & ((1ull << n) - 1);
}

// one thread per word of the caller's bitmaps: the bits of the reads that overlap it, fetched from the warm /
// cold bitmaps (over the compacted buffers, which are padded by one word)
__global__ __launch_bounds__(256) void merge_split_bitmaps_kernel(uint64_t n_words, uint64_t len, uint32_t L,
                                                                  const unsigned long long* flags, const uint32_t* prefix,
                                                                  const uint64_t* warm_hit, const uint64_t* cold_hit,
                                                                  const uint64_t* warm_valid, const uint64_t* cold_valid,
                                                                  uint64_t* hit_out, uint64_t* valid_out)
{
	const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (w >= n_words)
		return;
	uint64_t b0 = w * 64, b1 = b0 + 64;
	if (b1 > len)
		b1 = len;
	uint64_t hit = 0, valid = 0;
	for (uint64_t r = b0 / L; b0 < b1; ++r) {
		const uint64_t r_end = (r + 1) * L;
		const uint64_t e = r_end < b1 ? r_end : b1;
		const uint32_t n = (uint32_t)(e - b0);
		bool cold;
		const uint32_t rk = cold_rank(flags, prefix, r, &cold);
		const uint64_t src = (cold ? (uint64_t)rk : r - rk) * L + (b0 - r * L);
		const uint32_t sh = (uint32_t)(b0 - w * 64);
		if (hit_out)
			hit |= bits_at(cold ? cold_hit : warm_hit, src, n) << sh;
		if (valid_out)
			valid |= bits_at(cold ? cold_valid : warm_valid, src, n) << sh;
		b0 = e;
	}
	if (hit_out)
		hit_out[w] = hit;
	if (valid_out)
		valid_out[w] = valid;
}

// Only the cold reads are gathered (the split query's masked form: the warm reads stay where they are): one thread per
// read looks at its flag; a cold one copies its read to cold_buf[rank * L ..] in 16-byte steps and notes where it came
// from.  (compact_reads_kernel, one thread per 16-byte piece of EVERY read, spends its time finding out that 99 % of
// the pieces are not wanted.)
__global__ __launch_bounds__(256) void gather_cold_reads_kernel(const uint8_t* seq, uint64_t n_reads, uint32_t L,
                                                                const unsigned long long* flags, const uint32_t* prefix,
                                                                uint8_t* cold_buf, uint32_t* cold_index)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_reads)
		return;
	bool cold;
	const uint32_t rk = cold_rank(flags, prefix, r, &cold);
	if (!cold)
		return;
	cold_index[rk] = (uint32_t)r;
	const uint8_t* src = seq + r * L;
	uint8_t* dst = cold_buf + (uint64_t)rk * L;
	uint32_t i = 0;
	for (; i + 16 <= L; i += 16) {
		uint32_t w[4];
		__builtin_memcpy(w, src + i, 16); // unaligned loads / stores
		__builtin_memcpy(dst + i, w, 16);
	}
	for (; i + 4 <= L; i += 4) {
		uint32_t w;
		__builtin_memcpy(&w, src + i, 4);
		__builtin_memcpy(dst + i, &w, 4);
	}
	for (; i < L; ++i)
		dst[i] = src[i];
}

hipError_t launch_gather_cold_reads(const uint8_t* seq, uint64_t n_reads, uint32_t L, const uint64_t* flags,
                                    const uint32_t* prefix, uint8_t* cold_buf, uint32_t* cold_index, hipStream_t s)
{
	if (n_reads == 0)
		return hipSuccess;
	hipLaunchKernelGGL(gather_cold_reads_kernel, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, s, seq, n_reads, L,
	                   reinterpret_cast<const unsigned long long*>(flags), prefix, cold_buf, cold_index);
	return hipGetLastError();
}

// The cold reads' answers (bitmaps over the gathered cold buffer) go back to where the reads lie in the caller's
// buffer: one thread per cold read ORs its L bits into the caller's bitmaps, whose bits for that read pass A left zero.
__global__ __launch_bounds__(256) void merge_cold_bitmaps_kernel(uint64_t n_cold, uint32_t L, const uint32_t* cold_index,
                                                                 const uint64_t* cold_hit, const uint64_t* cold_valid,
                                                                 unsigned long long* hit_out, unsigned long long* valid_out)
{
	const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= n_cold)
		return;
	uint64_t src = c * L, dst = (uint64_t)cold_index[c] * L;
	for (uint32_t left = L; left;) {
		const uint32_t sh = (uint32_t)(dst & 63), n = left < 64 - sh ? left : 64 - sh;
		if (hit_out) {
			const uint64_t v = bits_at(cold_hit, src, n);
			if (v)
				atomicOr(&hit_out[dst >> 6], (unsigned long long)(v << sh));
		}
		if (valid_out) {
			const uint64_t v = bits_at(cold_valid, src, n);
			if (v)
				atomicOr(&valid_out[dst >> 6], (unsigned long long)(v << sh));
		}
		src += n;
		dst += n;
		left -= n;
	}
}

hipError_t launch_merge_cold_bitmaps(uint64_t n_cold, uint32_t L, const uint32_t* cold_index, const uint64_t* cold_hit,
                                     const uint64_t* cold_valid, uint64_t* hit_out, uint64_t* valid_out, hipStream_t s)
{
	if (n_cold == 0)
		return hipSuccess;
	hipLaunchKernelGGL(merge_cold_bitmaps_kernel, dim3((unsigned)((n_cold + 255) / 256)), dim3(256), 0, s, n_cold, L,
	                   cold_index, cold_hit, cold_valid, reinterpret_cast<unsigned long long*>(hit_out),
	                   reinterpret_cast<unsigned long long*>(valid_out));
	return hipGetLastError();
}

// stride > 1: only every stride-th read is sampled and only *n_cold is produced (a cheap estimate)
hipError_t launch_read_sample(const uint8_t* seq, uint64_t n_reads, uint32_t L, uint32_t stride, const HashParams& hp,
                              const ModParams& mod, const void* filter, int counting, uint32_t threshold, uint64_t* flags,
                              uint64_t* n_cold, hipStream_t s, uint32_t probes2)
{
	if (n_reads == 0 || stride == 0)
		return hipSuccess;
	if (probes2 == 0 || probes2 > hp.h)
		probes2 = hp.h;
	const uint64_t n_s = (n_reads + stride - 1) / stride;
	const size_t staged_bytes = (size_t)256 * L + 32;
	if (stride == 1 && staged_bytes <= 40 * 1024) { // every read looked at, and 256 of them fit the LDS (L <= 159)
		hipLaunchKernelGGL(read_sample_kernel<true>, dim3((unsigned)((n_s + 255) / 256)), dim3(256), staged_bytes, s, seq,
		                   n_reads, L, stride, hp, mod, filter, (uint32_t)counting, threshold, probes2,
		                   reinterpret_cast<unsigned long long*>(flags), reinterpret_cast<unsigned long long*>(n_cold));
		return hipGetLastError();
	}
	hipLaunchKernelGGL(read_sample_kernel<false>, dim3((unsigned)((n_s + 255) / 256)), dim3(256), 0, s, seq, n_reads, L, stride,
	                   hp, mod, filter, (uint32_t)counting, threshold, probes2, reinterpret_cast<unsigned long long*>(flags),
	                   reinterpret_cast<unsigned long long*>(n_cold));
	return hipGetLastError();
}

// prefix must hold ceil(n_reads / 64) uint32 + one uint32 per 1024 of those (scratch behind it)
hipError_t launch_flag_prefix(const uint64_t* flags, uint64_t n_reads, uint32_t* prefix, hipStream_t s)
{
	const uint64_t n_words = (n_reads + 63) / 64;
	if (n_words == 0)
		return hipSuccess;
	const uint32_t n_chunks = (uint32_t)((n_words + 1023) / 1024);
	uint32_t* chunk = prefix + n_words;
	const unsigned long long* fl = reinterpret_cast<const unsigned long long*>(flags);
	hipLaunchKernelGGL(flag_chunk_sum_kernel, dim3(n_chunks), dim3(1024), 0, s, fl, n_words, chunk);
	hipLaunchKernelGGL(flag_chunk_scan_kernel, dim3(1), dim3(64), 0, s, chunk, n_chunks);
	hipLaunchKernelGGL(flag_prefix_kernel, dim3(n_chunks), dim3(1024), 0, s, fl, n_words, chunk, prefix);
	return hipGetLastError();
}

hipError_t launch_compact_reads(const uint8_t* seq, uint64_t n_reads, uint32_t L, const uint64_t* flags,
                                const uint32_t* prefix, uint8_t* warm_buf, uint8_t* cold_buf, hipStream_t s)
{
	if (n_reads == 0)
		return hipSuccess;
	const uint32_t ppr = (L + 15) / 16; // 16-byte pieces per read
	const uint32_t ppr_inv = (uint32_t)(0xffffffffull / ppr) + 1; // floor(x / ppr) = umulhi(x, ppr_inv) for x < 2^16
	const uint32_t rpt = ppr > 256 ? 1u : 256u / ppr; // reads per workgroup and trip
	const uint64_t trips = (n_reads + rpt - 1) / rpt;
	const unsigned blocks = (unsigned)(trips < 65536 ? trips : 65536);
	hipLaunchKernelGGL(compact_reads_kernel, dim3(blocks), dim3(256), 0, s, seq, n_reads, L, ppr, ppr_inv,
	                   reinterpret_cast<const unsigned long long*>(flags), prefix, warm_buf, cold_buf);
	return hipGetLastError();
}

hipError_t launch_merge_split_bitmaps(uint64_t len, uint32_t L, const uint64_t* flags, const uint32_t* prefix,
                                      const uint64_t* warm_hit, const uint64_t* cold_hit, const uint64_t* warm_valid,
                                      const uint64_t* cold_valid, uint64_t* hit_out, uint64_t* valid_out, hipStream_t s)
{
	const uint64_t n_words = (len + 63) / 64;
	if (n_words == 0)
		return hipSuccess;
	hipLaunchKernelGGL(merge_split_bitmaps_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, s, n_words, len, L,
	                   reinterpret_cast<const unsigned long long*>(flags), prefix, warm_hit, cold_hit, warm_valid, cold_valid,
	                   hit_out, valid_out);
	return hipGetLastError();
}

} // namespace btlbf
