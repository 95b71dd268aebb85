// csrc/screen_kernels.hip -- the read screen: every read against several bit filters in one pass.
//   * screen_kernel<NF, SPACED>: seq_kernel's structure (seq_kernels.hip: 256 threads, tiles of 2048 window starts, 8
//     windows per lane, staging and hashing from seq_core.hpp) with NF filters behind one hash stage.  A clean window's h
//     values are computed once; each is reduced with every filter's own ModParams and tested in that filter's array.
//     Plain ntHash: probe 0 of all 8 windows x NF filters of a lane is issued in the window walk and consumed after it;
//     the probes 1..h-1 are issued, three hash values at a time, only for the (window, filter) pairs still alive --
//     OP_BF_CONTAINS's early exit, per filter.  Spaced seeds: a window's values are produced one at a time
//     (seq_strand_walk, as the wide-counter kernels do: no run-time-indexed array of them, so no scratch) and each is
//     tested in the filters still alive for that window.  The filter loop is unrolled on NF; per-filter state is either
//     a statically indexed register array or a bit of a mask.  A lane's 8 windows are one byte of every per-window
//     bitmap: NF hit columns and the valid column leave as coalesced byte stores.
//   * screen_reduce_kernel: the columns -> hits[row][filter] and valid[row], one lane per (row, column); a sequence of
//     more than kLaneWords bitmap words is counted by the lane's whole wave.
//   * screen_verdict_kernel: pass_bits[row]; screen_tally_kernel: the summary of rows added to running totals
//     (mibf_tally_kernel's pattern: wave reductions, one atomic per wave or, for the per-filter bins, per workgroup).
// Reference semantics: BloomFilter::contains (BloomFilter.hpp:247-262) of every k-mer of a read, per filter.
#include "seq_core.hpp"

#include <algorithm>
#include <type_traits>

namespace btlbf {

static constexpr int kScreenThreads = 256;
static constexpr int kScreenTile = kScreenThreads * kW;

// position of a hash value in filter m's array: the filters of one call may mix sizes that are and are not powers of
// two, and sizes above 2^32 bits (reduce_mod's other form); all three tests are uniform
__device__ __forceinline__ uint64_t screen_pos(uint64_t hash, const ModParams& m)
{
	return m.pow2 ? hash & m.mask : reduce_mod<false>(hash, m);
}

// f(std::integral_constant<int, I>) for I = I .. N-1: the second wave's window index is a constant without a loop to
// unroll (the compiler gives up on a pragma's full unroll of a body this size, and the lane's probe words, indexed by
// the loop counter then, go to scratch)
template <int I, int N, class F>
__device__ __forceinline__ void screen_each(F&& f)
{
	if constexpr (I < N) {
		f(std::integral_constant<int, I>{});
		screen_each<I + 1, N>(f);
	}
}

template <int NF, bool SPACED>
__global__ __launch_bounds__(kScreenThreads) void screen_kernel(const ScreenArgs a)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
	__shared__ SeqShared sh;

	const uint32_t tid = threadIdx.x;
	const uint32_t k = a.hp.k;
	const uint32_t h = a.hp.h;
	const uint32_t tile_cap = seq_tile_cap(kScreenTile, k);
	uint8_t* tile = dyn;
	uint8_t* spaced_lds = dyn + tile_cap;
	seq_setup_tables<kScreenThreads, SPACED>(sh, a.hp, spaced_lds);

	const uint64_t t_begin = (uint64_t)blockIdx.x * a.tiles_per_block;
	uint64_t t_end = t_begin + a.tiles_per_block;
	if (t_end > a.n_tiles)
		t_end = a.n_tiles;
	const uint32_t L = a.layout.starts ? 0 : a.layout.read_len;
	uint32_t tile_off = 0;
	if (L && t_begin < t_end)
		tile_off = (uint32_t)((t_begin * (uint64_t)kScreenTile) % L);
	const uint32_t tile_step = L ? (uint32_t)(kScreenTile % L) : 0;
	const uint64_t out_bytes = ((a.len + 63) / 64) * 8;

	for (uint64_t t = t_begin; t < t_end; ++t) {
		const uint64_t g0 = t * (uint64_t)kScreenTile;
		const uint32_t mis = seq_stage_tile<kScreenThreads>(tile, tile_cap, sh, a.seq, a.len, a.layout, k, g0, tile_off);
		tile_off = seq_next_tile_off(tile_off, tile_step, L);

		uint32_t valid_mask = 0;
		uint32_t hit[NF]; // bit w = window w of the lane is in filter j
#pragma unroll
		for (int j = 0; j < NF; ++j)
			hit[j] = 0;

		if constexpr (SPACED) {
			const uint32_t li0 = tid * kW + mis;
			const uint8_t* bp = tile + li0;
			const uint16_t* dc_idx = reinterpret_cast<const uint16_t*>(spaced_lds + seq_pos_tab_bytes(a.hp));
			const uint32_t n_seeds = a.hp.n_seeds, h2 = a.hp.h2;
			LaneState st;
			seq_strand_walk<0>(tile, sh, k, a.hp.kms, li0, st, [&](int w, bool ok, uint64_t fh, uint64_t rh) {
				valid_mask |= (uint32_t)ok << w;
				uint32_t alive = ok ? (1u << NF) - 1u : 0u; // bit j: every value so far found its bit set in filter j
				// one value in the filters still alive: their loads go out together
				auto probe = [&](uint64_t hv) {
					uint32_t wd[NF], bt[NF];
#pragma unroll
					for (int j = 0; j < NF; ++j) {
						wd[j] = bt[j] = 0;
						if ((alive >> j) & 1u) {
							const uint64_t p = screen_pos(hv, a.mod[j]);
							wd[j] = bf_word(a.words[j], p);
							bt[j] = (uint32_t)p & 31;
						}
					}
#pragma unroll
					for (int j = 0; j < NF; ++j)
						alive &= ~(1u << j) | (((wd[j] >> bt[j]) & 1u) << j);
				};
				// value j * h2 + j2 is extra hash j2 of seed j's base value: the window's strand hashes with the terms of
				// the seed's don't-care positions XORed back out, the smaller strand (seq_core.hpp's per-seed walk)
				for (uint32_t j = 0; j < n_seeds && alive; ++j) {
					uint64_t fs = fh, rs = rh;
					for (uint32_t d = a.hp.dc_off[j]; d < a.hp.dc_off[j + 1]; ++d) {
						const uint32_t di = dc_idx[d];
						const U64x2 tt = tab16(spaced_lds, di * (kNumCodes * 16) + (bp[w + di] & kCodeOff));
						fs ^= tt.x;
						rs ^= tt.y;
					}
					const uint64_t b = rs < fs ? rs : fs;
					probe(b);
					for (uint32_t j2 = 1; j2 < h2 && alive; ++j2)
						probe(extra_hash(b, a.hp.kms, j2));
				}
#pragma unroll
				for (int j = 0; j < NF; ++j)
					hit[j] |= ((alive >> j) & 1u) << w;
			});
		} else {
			// first wave of loads: probe 0 of every window in every filter (a window that is not clean asks for nothing)
			uint32_t word0[kW][NF];
			uint64_t bit0[kW]; // 5 bits per filter: the bit of word0[w][j] that counts
			uint64_t canon[kW];
			seq_lane_windows<false, kW>(tile, sh, a.hp, spaced_lds, tid * kW + mis, [&](int w, bool ok, const WinHash<false>& wh) {
				valid_mask |= (uint32_t)ok << w;
				canon[w] = wh.bcan;
				bit0[w] = 0;
#pragma unroll
				for (int j = 0; j < NF; ++j) {
					word0[w][j] = 0;
					if (ok) {
						const uint64_t p = screen_pos(wh.bcan, a.mod[j]);
						word0[w][j] = bf_word(a.words[j], p);
						bit0[w] |= (uint64_t)((uint32_t)p & 31) << (5 * j);
					}
				}
			});
			// second wave, window by window: the values 1..h-1, kStep at a time, in the filters still alive
			constexpr int kStep = 3;
			screen_each<0, kW>([&](auto wc) {
				constexpr int w = decltype(wc)::value;
				uint32_t alive = 0;
#pragma unroll
				for (int j = 0; j < NF; ++j)
					alive |= ((word0[w][j] >> ((uint32_t)(bit0[w] >> (5 * j)) & 31)) & 1u) << j;
				for (uint32_t i0 = 1; i0 < h && alive; i0 += kStep) {
					uint64_t hv[kStep];
#pragma unroll
					for (int c = 0; c < kStep; ++c)
						hv[c] = extra_hash(canon[w], a.hp.kms, i0 + c);
					uint32_t wd[NF][kStep], bt[NF][kStep];
#pragma unroll
					for (int j = 0; j < NF; ++j) {
#pragma unroll
						for (int c = 0; c < kStep; ++c) {
							wd[j][c] = 0xffffffffu; // a value that is not there (i0 + c >= h) or not asked for changes nothing
							bt[j][c] = 0;
						}
						if ((alive >> j) & 1u) {
#pragma unroll
							for (int c = 0; c < kStep; ++c) {
								if (i0 + c < h) {
									const uint64_t p = screen_pos(hv[c], a.mod[j]);
									wd[j][c] = bf_word(a.words[j], p);
									bt[j][c] = (uint32_t)p & 31;
								}
							}
						}
					}
#pragma unroll
					for (int j = 0; j < NF; ++j) {
						uint32_t all = 1;
#pragma unroll
						for (int c = 0; c < kStep; ++c)
							all &= wd[j][c] >> bt[j][c];
						alive &= ~(1u << j) | ((all & 1u) << j);
					}
				}
#pragma unroll
				for (int j = 0; j < NF; ++j)
					hit[j] |= ((alive >> j) & 1u) << w;
			});
		}

		// ---- results: one byte per column ----
		const uint64_t ob = (g0 >> 3) + tid;
		if (ob < out_bytes) {
#pragma unroll
			for (int j = 0; j < NF; ++j)
				a.hit_cols[(uint64_t)j * a.col_bytes + ob] = (uint8_t)hit[j];
			if (a.valid_bits)
				a.valid_bits[ob] = (uint8_t)valid_mask;
		}
	}
}

template <int NF>
static hipError_t screen_launch_nf(const ScreenArgs& a, hipStream_t s, dim3 grid, size_t dyn)
{
#define BTLBF_SCREEN_LAUNCH(S)                                                                               \
	do {                                                                                                     \
		if (dyn > 48 * 1024) {                                                                               \
			hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&screen_kernel<NF, S>),          \
			                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);         \
			if (e != hipSuccess)                                                                             \
				return e;                                                                                    \
		}                                                                                                    \
		hipLaunchKernelGGL((screen_kernel<NF, S>), grid, dim3(kScreenThreads), dyn, s, a);                   \
	} while (0)
	if (a.hp.n_seeds > 0)
		BTLBF_SCREEN_LAUNCH(true);
	else
		BTLBF_SCREEN_LAUNCH(false);
#undef BTLBF_SCREEN_LAUNCH
	return hipGetLastError();
}

// the whole buffer in one launch: a few workgroups per CU, each walking a contiguous run of tiles (launch_seq_op's grid)
hipError_t launch_screen(const ScreenArgs& a_in, hipStream_t s)
{
	ScreenArgs a = a_in;
	if (a.len == 0)
		return hipSuccess;
	if (a.nf == 0 || a.nf > kScreenMaxNF || !a.hit_cols)
		return hipErrorInvalidValue;
	a.n_tiles = (a.len + kScreenTile - 1) / kScreenTile;
	int dev = 0, cus = 256;
	if (hipGetDevice(&dev) == hipSuccess) {
		int v = 0;
		if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
			cus = v;
	}
	const uint64_t max_blocks = (uint64_t)cus * 8;
	uint64_t blocks = a.n_tiles < max_blocks ? a.n_tiles : max_blocks;
	a.tiles_per_block = (a.n_tiles + blocks - 1) / blocks;
	blocks = (a.n_tiles + a.tiles_per_block - 1) / a.tiles_per_block;
	static_assert(kScreenTile == (int)kSeqTileWindows, "seq_lds_dyn counts this kernel's tile");
	if (!seq_lds_fits(a.hp)) // (build_spaced refuses such seeds with a message; nothing is launched or configured here)
		return hipErrorInvalidValue;
	const size_t dyn = seq_lds_dyn(a.hp);
	const dim3 grid((unsigned)blocks);
	switch (a.nf) {
	case 1: return screen_launch_nf<1>(a, s, grid, dyn);
	case 2: return screen_launch_nf<2>(a, s, grid, dyn);
	case 3: return screen_launch_nf<3>(a, s, grid, dyn);
	case 4: return screen_launch_nf<4>(a, s, grid, dyn);
	case 5: return screen_launch_nf<5>(a, s, grid, dyn);
	case 6: return screen_launch_nf<6>(a, s, grid, dyn);
	case 7: return screen_launch_nf<7>(a, s, grid, dyn);
	default: return screen_launch_nf<8>(a, s, grid, dyn);
	}
}

// ---- columns -> per-row counts ---------------------------------------------------------------------------------
// set bits of `bits` in the window range [lo, hi) (bit p = the window that starts at byte p), over the words
// first, first + step, ... of the range's words [lo / 64, (hi - 1) / 64]
__device__ __forceinline__ uint32_t screen_popc(const uint64_t* bits, uint64_t lo, uint64_t hi, uint64_t first, uint64_t step)
{
	uint32_t n = 0;
	const uint64_t w0 = lo >> 6, w1 = (hi - 1) >> 6;
	for (uint64_t w = first; w <= w1; w += step) {
		uint64_t x = bits[w];
		if (w == w0)
			x &= ~0ull << (lo & 63);
		if (w == w1 && (hi & 63) != 0)
			x &= ~0ull >> (64 - (hi & 63));
		n += __popcll(x);
	}
	return n;
}

static constexpr uint32_t kLaneWords = 8; // a range of up to this many bitmap words is counted by its own lane

__global__ __launch_bounds__(256) void screen_reduce_kernel(const uint64_t* cols, uint64_t col_words, uint64_t len,
                                                            const uint64_t* starts, uint64_t n_rows, uint32_t read_len,
                                                            uint32_t k, uint32_t nf, uint32_t* hits, uint32_t* valid)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t items = n_rows * (nf + 1); // item = row * (nf + 1) + column; column nf is the valid bitmap
	// (the trip count is uniform over a wave: the long ranges below are counted by all 64 lanes)
	for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < items;
	     base += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t it = base + lane;
		const bool act = it < items;
		const uint64_t row = act ? it / (nf + 1) : 0;
		const uint32_t c = act ? (uint32_t)(it - row * (nf + 1)) : 0;
		// the row's windows start in [b, hi): btlbf_count_per_seq's range
		uint64_t b = 0, e = len;
		if (starts) {
			b = starts[row];
			e = starts[row + 1];
		} else if (read_len) {
			b = row * read_len;
			e = b + read_len;
		}
		if (e > len)
			e = len;
		const uint64_t hi = e >= b + k ? e - k + 1 : b;
		const uint64_t words = act && hi > b ? ((hi - 1) >> 6) - (b >> 6) + 1 : 0;
		const uint64_t* bits = cols + (uint64_t)c * col_words;
		uint32_t n = 0;
		if (words && words <= kLaneWords)
			n = screen_popc(bits, b, hi, b >> 6, 1);
		uint64_t todo = __ballot(words > kLaneWords);
		while (todo) {
			const int src = __ffsll((unsigned long long)todo) - 1;
			todo &= todo - 1;
			const uint64_t sb = __shfl(b, src, 64), shi = __shfl(hi, src, 64);
			const uint32_t sc = __shfl(c, src, 64);
			const uint32_t part = wave_sum(screen_popc(cols + (uint64_t)sc * col_words, sb, shi, (sb >> 6) + lane, 64));
			if ((int)lane == src)
				n = part;
		}
		if (act) {
			if (c < nf)
				hits[row * nf + c] = n;
			else
				valid[row] = n;
		}
	}
}

hipError_t launch_screen_reduce(const uint64_t* cols, uint64_t col_words, uint64_t len, const LayoutParams& lay,
                                uint64_t n_rows, uint32_t k, uint32_t n_filters, uint32_t* hits, uint32_t* valid,
                                hipStream_t s)
{
	if (n_rows == 0)
		return hipSuccess;
	const uint64_t items = n_rows * (n_filters + 1);
	const uint64_t blocks = std::min<uint64_t>((items + 255) / 256, 65536);
	hipLaunchKernelGGL(screen_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, cols, col_words, len, lay.starts,
	                   n_rows, lay.starts ? 0u : lay.read_len, k, n_filters, hits, valid);
	return hipGetLastError();
}

// ---- the row verdict ---------------------------------------------------------------------------------------------
// bit j: the row has clean windows, at least min_hits of them in filter j, and at least min_fraction of them (one IEEE
// double multiply and one compare)
__global__ __launch_bounds__(256) void screen_verdict_kernel(const uint32_t* hits, const uint32_t* valid, uint64_t n_rows,
                                                             uint32_t nf, double min_fraction, uint32_t min_hits,
                                                             uint32_t* pass_bits)
{
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t v = valid[r];
		const double need = min_fraction * (double)v;
		uint32_t bits = 0;
		for (uint32_t j = 0; j < nf; ++j) {
			const uint32_t hj = hits[r * nf + j];
			bits |= (uint32_t)(v > 0 && hj >= min_hits && (double)hj >= need) << j;
		}
		pass_bits[r] = bits;
	}
}

hipError_t launch_screen_verdict(const uint32_t* hits, const uint32_t* valid, uint64_t n_rows, uint32_t n_filters,
                                 double min_fraction, uint32_t min_hits, uint32_t* pass_bits, hipStream_t s)
{
	if (n_rows == 0)
		return hipSuccess;
	const uint64_t blocks = std::min<uint64_t>((n_rows + 255) / 256, 65536);
	hipLaunchKernelGGL(screen_verdict_kernel, dim3((unsigned)blocks), dim3(256), 0, s, hits, valid, n_rows, n_filters,
	                   min_fraction, min_hits, pass_bits);
	return hipGetLastError();
}

// ---- the summary of rows -----------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long screen_wave_sum64(unsigned long long v)
{
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}

__global__ __launch_bounds__(256) void screen_tally_kernel(const uint32_t* hits, const uint32_t* valid,
                                                           const uint32_t* pass_bits, uint64_t n_rows, uint32_t nf,
                                                           unsigned long long* passed, unsigned long long* best,
                                                           unsigned long long* totals4, unsigned long long* windows)
{
	__shared__ uint32_t bins[2 * kScreenMaxFilters]; // passed, then best
	if (threadIdx.x < 2 * kScreenMaxFilters)
		bins[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63;
	uint32_t rows = 0, none = 0, multi = 0, empty = 0;
	unsigned long long win = 0;
	// (uniform trip count over a wave: the per-filter counts are ballots)
	for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n_rows;
	     base += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t r = base + lane;
		const bool act = r < n_rows;
		const uint32_t pb = act ? pass_bits[r] & (nf < 32 ? (1u << nf) - 1u : ~0u) : 0u;
		const uint32_t v = act ? valid[r] : 1u;
		rows += act;
		none += act && pb == 0;
		multi += __popc(pb) > 1;
		empty += v == 0;
		win += act ? v : 0u;
		// the passing filter with the most hits, ties to the lowest index
		uint32_t bj = nf, bh = 0;
		for (uint32_t j = 0; j < nf; ++j) {
			if ((pb >> j) & 1u) {
				const uint32_t hj = hits[r * nf + j];
				if (bj == nf || hj > bh) {
					bj = j;
					bh = hj;
				}
			}
		}
		for (uint32_t j = 0; j < nf; ++j) {
			const uint32_t np = __popcll(__ballot((pb >> j) & 1u)), nb = __popcll(__ballot(bj == j));
			if (lane == 0 && np)
				atomicAdd(bins + j, np);
			if (lane == 0 && nb)
				atomicAdd(bins + kScreenMaxFilters + j, nb);
		}
	}
	rows = wave_sum(rows);
	none = wave_sum(none);
	multi = wave_sum(multi);
	empty = wave_sum(empty);
	win = screen_wave_sum64(win);
	if (lane == 0 && rows) {
		atomicAdd(totals4 + 0, (unsigned long long)rows);
		if (none)
			atomicAdd(totals4 + 1, (unsigned long long)none);
		if (multi)
			atomicAdd(totals4 + 2, (unsigned long long)multi);
		if (empty)
			atomicAdd(totals4 + 3, (unsigned long long)empty);
		if (windows && win)
			atomicAdd(windows, win);
	}
	__syncthreads();
	if (threadIdx.x < nf) {
		if (bins[threadIdx.x])
			atomicAdd(passed + threadIdx.x, (unsigned long long)bins[threadIdx.x]);
		if (bins[kScreenMaxFilters + threadIdx.x])
			atomicAdd(best + threadIdx.x, (unsigned long long)bins[kScreenMaxFilters + threadIdx.x]);
	}
}

hipError_t launch_screen_tally(const uint32_t* hits, const uint32_t* valid, const uint32_t* pass_bits, uint64_t n_rows,
                               uint32_t n_filters, unsigned long long* passed, unsigned long long* best,
                               unsigned long long* totals4, unsigned long long* windows, hipStream_t s)
{
	if (n_rows == 0)
		return hipSuccess;
	const uint64_t blocks = std::min<uint64_t>((n_rows + 255) / 256, 512);
	hipLaunchKernelGGL(screen_tally_kernel, dim3((unsigned)blocks), dim3(256), 0, s, hits, valid, pass_bits, n_rows,
	                   n_filters, passed, best, totals4, windows);
	return hipGetLastError();
}

} // namespace btlbf
