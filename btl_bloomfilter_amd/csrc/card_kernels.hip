// csrc/card_kernels.hip -- the k-mer cardinality sketch (include/btlbf.h: btlbf_card_*).
//   * card_kernel: screen_kernel's structure (screen_kernels.hip: 256 threads, tiles of 2048 window starts, 8 windows per
//     lane, staging and hashing from seq_core.hpp) without a probe stage.  A clean window's canonical hash is mixed
//     (mix64), tested against the sampling mask, and a sampled window is one atomicAdd on its counter.  The clean and the
//     sampled windows are counted per wave (ballot, popcount), summed per workgroup in LDS and added with one atomic each
//     per workgroup; the windows -- k bytes inside one sequence, whatever they hold -- follow from the layout alone and
//     are summed by the same launch over the sequences' lengths.
//     Saturation: the add is unconditional, so a counter at 2^32 - 1 wraps to 0 -- and the one add that does that sees
//     the old value 2^32 - 1 and sets the counter's bit in `wrapped`.  card_fix_kernel, launched behind on the same
//     stream, stores 2^32 - 1 into every marked counter and clears the bitmap again.  A counter's true value passed the
//     maximum iff it was marked, whatever the order of the adds and however many there were, so no counter is ever seen
//     wrapped by a later launch and nothing depends on how many adds are in flight at once.
//   * card_hist_kernel: t[min(c, n_hist - 1)] += 1 over the counters c, one streaming pass of 16-byte loads.  A per-block
//     LDS histogram, flushed with 64-bit atomics; the zero counters -- nearly all of a table in its working range -- are
//     counted per wave by ballot and reach the LDS bin once per wave.
//   * card_merge_kernel: dst = min(dst + src, 2^32 - 1) per counter, the totals added.
#include "seq_core.hpp"

#include <algorithm>

namespace btlbf {

static constexpr int kCardThreads = 256;
static constexpr int kCardTile = kCardThreads * kW;
static constexpr uint32_t kCardMax = 0xffffffffu;

__global__ __launch_bounds__(kCardThreads) void card_kernel(const CardArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
	__shared__ SeqShared sh;
	__shared__ uint32_t blk_cnt[2]; // clean, sampled windows of this workgroup (a workgroup walks fewer than 2^32)

	const uint32_t tid = threadIdx.x;
	const uint32_t lane = tid & 63;
	const uint32_t k = a.hp.k;
	const uint32_t tile_cap = seq_tile_cap(kCardTile, k);
	uint8_t* tile = dyn;
	uint8_t* tables = dyn + tile_cap;
	seq_setup_tables<kCardThreads, false>(sh, a.hp, tables);
	if (tid < 2)
		blk_cnt[tid] = 0; // (the first tile's staging has the barrier)

	const uint64_t t_begin = (uint64_t)blockIdx.x * a.tiles_per_block;
	uint64_t t_end = t_begin + a.tiles_per_block;
	if (t_end > a.n_tiles)
		t_end = a.n_tiles;
	const uint32_t L = a.layout.starts ? 0 : a.layout.read_len;
	uint32_t tile_off = 0;
	if (L && t_begin < t_end)
		tile_off = (uint32_t)((t_begin * (uint64_t)kCardTile) % L);
	const uint32_t tile_step = L ? (uint32_t)(kCardTile % L) : 0;
	// sampled iff the top sample_bits bits of the mixed value are zero
	const uint64_t top = a.sample_bits ? ~0ull << (64 - a.sample_bits) : 0ull;
	const uint64_t low = (1ull << a.table_bits) - 1;
	uint32_t n_clean = 0, n_sampled = 0; // of the wave: uniform

	for (uint64_t t = t_begin; t < t_end; ++t) {
		const uint64_t g0 = t * (uint64_t)kCardTile;
		const uint32_t mis = seq_stage_tile<kCardThreads>(tile, tile_cap, sh, a.seq, a.len, a.layout, k, g0, tile_off);
		tile_off = seq_next_tile_off(tile_off, tile_step, L);
		seq_lane_windows<false, kW>(tile, sh, a.hp, tables, tid * kW + mis, [&](int, bool ok, const WinHash<false>& wh) {
			const uint64_t z = mix64(wh.bcan);
			const bool take = ok && (z & top) == 0;
			n_clean += __popcll(__ballot(ok));
			n_sampled += __popcll(__ballot(take));
			if (take) {
				const uint32_t b = (uint32_t)(z & low);
				if (atomicAdd(a.table + b, 1u) == kCardMax)
					atomicOr(a.wrapped + (b >> 5), 1u << (b & 31));
			}
		});
	}
	if (lane == 0 && n_clean) {
		atomicAdd(&blk_cnt[0], n_clean);
		if (n_sampled)
			atomicAdd(&blk_cnt[1], n_sampled);
	}

	// the windows: sum over the sequences of max(0, length - k + 1)
	unsigned long long win = 0;
	const uint64_t gid = (uint64_t)blockIdx.x * kCardThreads + tid, gstep = (uint64_t)gridDim.x * kCardThreads;
	if (a.layout.starts) {
		for (uint64_t i = gid; i < a.layout.n_seqs; i += gstep) {
			const uint64_t b = a.layout.starts[i];
			uint64_t e = a.layout.starts[i + 1];
			if (e > a.len)
				e = a.len;
			if (e >= b + k)
				win += e - b - k + 1;
		}
	} else if (gid == 0) {
		if (L)
			win = L >= k ? (a.len / L) * (uint64_t)(L - k + 1) : 0;
		else
			win = a.len >= k ? a.len - k + 1 : 0;
	}
	for (int o = 32; o > 0; o >>= 1)
		win += __shfl_xor(win, o, 64);
	if (lane == 0 && win)
		atomicAdd(a.totals3 + 0, win);
	__syncthreads();
	if (tid < 2 && blk_cnt[tid])
		atomicAdd(a.totals3 + 1 + tid, (unsigned long long)blk_cnt[tid]);
}

// counters marked in `wrapped` (words of 32 bits, bit b & 31 of word b >> 5) go back to the maximum; the bitmap is zero again
__global__ __launch_bounds__(256) void card_fix_kernel(uint32_t* table, uint32_t* wrapped, uint32_t n_words)
{
	for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += gridDim.x * blockDim.x) {
		uint32_t m = wrapped[w];
		if (m == 0)
			continue;
		wrapped[w] = 0;
		while (m) {
			const uint32_t b = (uint32_t)__ffs((int)m) - 1;
			m &= m - 1;
			table[(w << 5) + b] = kCardMax;
		}
	}
}

hipError_t launch_card(const CardArgs& a_in, hipStream_t s)
{
	CardArgs a = a_in;
	if (a.len == 0)
		return hipSuccess;
	if (a.hp.n_seeds != 0 || a.table_bits < kCardMinTableBits || a.table_bits > kCardMaxTableBits ||
	    a.sample_bits > kCardMaxSampleBits || !a.table || !a.wrapped || !a.totals3)
		return hipErrorInvalidValue;
	a.n_tiles = (a.len + kCardTile - 1) / kCardTile;
	int dev = 0, cus = 256;
	if (hipGetDevice(&dev) == hipSuccess) {
		int v = 0;
		if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
			cus = v;
	}
	// a few workgroups per CU, each walking a contiguous run of tiles (launch_screen's grid)
	const uint64_t max_blocks = (uint64_t)cus * 8;
	uint64_t blocks = a.n_tiles < max_blocks ? a.n_tiles : max_blocks;
	a.tiles_per_block = (a.n_tiles + blocks - 1) / blocks;
	blocks = (a.n_tiles + a.tiles_per_block - 1) / a.tiles_per_block;
	static_assert(kCardTile == (int)kSeqTileWindows, "seq_lds_dyn counts this kernel's tile");
	if (!seq_lds_fits(a.hp))
		return hipErrorInvalidValue;
	const size_t dyn = seq_lds_dyn(a.hp);
	if (dyn > 48 * 1024) {
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&card_kernel),
		                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
		if (e != hipSuccess)
			return e;
	}
	hipLaunchKernelGGL(card_kernel, dim3((unsigned)blocks), dim3(kCardThreads), dyn, s, a);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	const uint32_t n_words = 1u << (a.table_bits - 5);
	hipLaunchKernelGGL(card_fix_kernel, dim3(std::min<uint32_t>((n_words + 255) / 256, 1024u)), dim3(256), 0, s, a.table,
	                   a.wrapped, n_words);
	return hipGetLastError();
}

// ---- the histogram of the counters -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void card_hist_kernel(const uint4* __restrict__ table, uint32_t n_vec, uint32_t n_hist,
                                                        unsigned long long* t)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
	uint32_t* bins = reinterpret_cast<uint32_t*>(dyn); // n_hist of them: a workgroup counts fewer than 2^32 counters
	for (uint32_t i = threadIdx.x; i < n_hist; i += blockDim.x)
		bins[i] = 0;
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t last = n_hist - 1;
	uint32_t zeros = 0; // of the wave: uniform
	// (a uniform trip count over a wave: the zero counters are ballots)
	for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n_vec; base += gridDim.x * blockDim.x) {
		const uint32_t i = base + lane;
		const bool act = i < n_vec;
		uint4 v = make_uint4(1u, 1u, 1u, 1u); // (a lane past the end counts nowhere)
		if (act)
			v = table[i];
		const uint32_t c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			zeros += __popcll(__ballot(c[q] == 0));
			if (act && c[q] != 0)
				atomicAdd(bins + (c[q] < last ? c[q] : last), 1u);
		}
	}
	if (lane == 0 && zeros)
		atomicAdd(bins + 0, zeros);
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < n_hist; i += blockDim.x)
		if (bins[i])
			atomicAdd(t + i, (unsigned long long)bins[i]);
}

hipError_t launch_card_hist(const uint32_t* table, uint32_t table_bits, uint32_t n_hist, unsigned long long* t, hipStream_t s)
{
	if (table_bits < kCardMinTableBits || table_bits > kCardMaxTableBits || n_hist < kCardMinHist || n_hist > kCardMaxHist ||
	    !table || !t)
		return hipErrorInvalidValue;
	const uint32_t n_vec = 1u << (table_bits - 2);
	// at most 1024 workgroups: each flushes up to n_hist atomics
	const uint32_t blocks = std::min<uint32_t>((n_vec + 255) / 256, 1024u);
	hipLaunchKernelGGL(card_hist_kernel, dim3(blocks), dim3(256), n_hist * sizeof(uint32_t), s,
	                   reinterpret_cast<const uint4*>(table), n_vec, n_hist, t);
	return hipGetLastError();
}

// ---- merge -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t card_sat_add(uint32_t a, uint32_t b)
{
	const uint32_t s = a + b;
	return s < a ? kCardMax : s;
}

__global__ __launch_bounds__(256) void card_merge_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, uint32_t n_vec,
                                                         unsigned long long* dst_tot, const unsigned long long* src_tot)
{
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += gridDim.x * blockDim.x) {
		const uint4 a = dst[i], b = src[i];
		dst[i] = make_uint4(card_sat_add(a.x, b.x), card_sat_add(a.y, b.y), card_sat_add(a.z, b.z), card_sat_add(a.w, b.w));
	}
	if (blockIdx.x == 0 && threadIdx.x < 3)
		dst_tot[threadIdx.x] += src_tot[threadIdx.x];
}

hipError_t launch_card_merge(uint32_t* dst, const uint32_t* src, uint32_t table_bits, unsigned long long* dst_totals3,
                             const unsigned long long* src_totals3, hipStream_t s)
{
	if (table_bits < kCardMinTableBits || table_bits > kCardMaxTableBits || !dst || !src || !dst_totals3 || !src_totals3)
		return hipErrorInvalidValue;
	const uint32_t n_vec = 1u << (table_bits - 2);
	const uint32_t blocks = std::min<uint32_t>((n_vec + 255) / 256, 4096u);
	hipLaunchKernelGGL(card_merge_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<uint4*>(dst),
	                   reinterpret_cast<const uint4*>(src), n_vec, dst_totals3, src_totals3);
	return hipGetLastError();
}

} // namespace btlbf
