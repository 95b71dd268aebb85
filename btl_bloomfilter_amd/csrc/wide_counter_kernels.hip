// csrc/wide_counter_kernels.hip -- counting filters with 16-, 32- and 64-bit counters (CountingBloomFilter<T>,
// CountingBloomFilter.hpp:26-111, T wider than a byte), direct path only:
//   * wide_seq_kernel: the fused sequence kernel -- stage, ntHash / spaced seeds, h probes, results in one launch --
//     built on seq_core.hpp exactly as seq_kernel is (seq_kernels.hip): 256 threads, 8 windows per lane, one byte of the
//     per-window bitmaps per lane, the same `counts` reduction.  Ops: query (hit bit, optional full-width minimum),
//     incrementAll, incrementMin.  With spaced seeds the h values of a window are produced and probed one at a time
//     (seq_core.hpp: seq_strand_walk), so that no instantiation keeps a run-time-indexed array of them in scratch memory;
//   * hash-row kernels, one lane per row or one lane in all (strict order), as aux_kernels.hip has them for bytes;
//   * reductions: non-zero counters, counters >= threshold, the three-way compare of two arrays.
// The width is a template parameter everywhere (wide_counter.hpp); the hash count stays a run-time value.  Positions are
// hash % (number of counters), CountingBloomFilter.hpp:56-58.  No shards: a wide filter is always whole.
#include "seq_core.hpp"
#include "wide_counter.hpp"

namespace btlbf {

static constexpr int kWideThreads = 256;
static constexpr int kWideTile = kWideThreads * kW;

template <int OP, int BYTES, bool POW2, bool SPACED>
__global__ __launch_bounds__(kWideThreads) void wide_seq_kernel(const SeqArgs a)
{
	using C = WideCtr<BYTES>;
	using V = typename C::V;
	extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
	__shared__ SeqShared sh;

	const uint32_t tid = threadIdx.x;
	const uint32_t k = a.hp.k;
	const uint32_t h = a.hp.h;
	const uint32_t tile_cap = seq_tile_cap(kWideTile, k);
	uint8_t* tile = dyn;
	uint8_t* spaced_lds = dyn + tile_cap;
	seq_setup_tables<kWideThreads, SPACED>(sh, a.hp, spaced_lds);

	const uint64_t t_begin = a.first_tile + (uint64_t)blockIdx.x * a.tiles_per_block;
	uint64_t t_end = t_begin + a.tiles_per_block;
	if (t_end > a.first_tile + a.n_tiles)
		t_end = a.first_tile + a.n_tiles;
	const uint32_t L = a.layout.starts ? 0 : a.layout.read_len;
	uint32_t tile_off = 0;
	if (L && t_begin < t_end)
		tile_off = (uint32_t)((t_begin * (uint64_t)kWideTile) % L);
	const uint32_t tile_step = L ? (uint32_t)(kWideTile % L) : 0;
	const uint64_t out_bytes = ((a.len + 63) / 64) * 8;

	uint32_t my_valid = 0, my_hit = 0;

	for (uint64_t t = t_begin; t < t_end; ++t) {
		const uint64_t g0 = t * (uint64_t)kWideTile;
		const uint32_t mis = seq_stage_tile<kWideThreads>(tile, tile_cap, sh, a.seq, a.len, a.layout, k, g0, tile_off);
		tile_off = seq_next_tile_off(tile_off, tile_step, L);

		uint32_t valid_mask = 0, hit_mask = 0;
		// query with <= kPipe hashes: the kW * h counter loads of a lane are issued in the window walk and consumed
		// after it (one memory latency per lane, not one per counter), as seq_kernel's pipelined paths do
		constexpr int kPipe = 4;
		V vals[kW][kPipe];
		(void)vals;
		const bool piped = (OP == W_QUERY) && !SPACED && h <= kPipe;

		// one window: `each_pos(g)` calls g(p) for the counter index p of each of the window's h hashes, in hash order
		auto window = [&](int w, bool ok, auto&& each_pos) {
			valid_mask |= (uint32_t)ok << w;
			const uint64_t gp = g0 + tid * kW + w; // byte offset of this window
			if (OP == W_QUERY) {
				V mn = C::kMax;
				if (ok) {
					each_pos([&](uint64_t p) {
						const V v = C::load(a.filter, p);
						mn = v < mn ? v : mn;
					});
					hit_mask |= (uint32_t)(mn >= (V)a.threshold) << w;
				}
				if (a.min_out && gp < a.len)
					wide_store<BYTES>(a.min_out, gp, ok ? mn : (V)0);
			} else if (OP == W_INC_ALL) {
				if (ok)
					each_pos([&](uint64_t p) { C::inc_sat(a.filter, p); });
			} else if (OP == W_INC_MIN) {
				if (ok)
					wide_increment_min<BYTES>(a.filter, each_pos);
			}
		};

		if constexpr (SPACED) {
			// Spaced seeds (stHashIterator): hash j * h2 + j2 is extra hash j2 of seed j's base value, and that is the
			// window's forward / reverse hash with the terms of the seed's don't-care positions XORed back out, the smaller
			// of the two strands (seq_core.hpp's per-seed walk).  The values are produced one at a time and probed at once --
			// no array of h values per window, which with a run-time h would live in scratch memory.  The window's two
			// strand hashes come from the plain-ntHash walk of seq_core.hpp, taken one window at a time through LaneState
			// (Horner start-up: the positional table in LDS has the single-base layout the don't-care terms need)
			const uint32_t li0 = tid * kW + mis;
			const uint8_t* bp = tile + li0;
			const uint16_t* dc_idx = reinterpret_cast<const uint16_t*>(spaced_lds + seq_pos_tab_bytes(a.hp));
			const uint32_t n_seeds = a.hp.n_seeds, h2 = a.hp.h2;
			LaneState st;
			seq_strand_walk<0>(tile, sh, k, a.hp.kms, li0, st, [&](int w, bool ok, uint64_t fh, uint64_t rh) {
				window(w, ok, [&](auto&& g) {
					for (uint32_t j = 0; j < n_seeds; ++j) {
						uint64_t fs = fh, rs = rh;
						for (uint32_t d = a.hp.dc_off[j]; d < a.hp.dc_off[j + 1]; ++d) {
							const uint32_t di = dc_idx[d];
							const U64x2 tt = tab16(spaced_lds, di * (kNumCodes * 16) + (bp[w + di] & kCodeOff));
							fs ^= tt.x;
							rs ^= tt.y;
						}
						const uint64_t b = rs < fs ? rs : fs;
						g(reduce_mod<POW2>(b, a.mod));
						for (uint32_t j2 = 1; j2 < h2; ++j2)
							g(reduce_mod<POW2>(extra_hash(b, a.hp.kms, j2), a.mod));
					}
				});
			});
		} else {
			seq_lane_windows<false, kW>(tile, sh, a.hp, spaced_lds, tid * kW + mis, [&](int w, bool ok, const WinHash<false>& wh) {
				if (OP == W_QUERY && piped) {
					valid_mask |= (uint32_t)ok << w;
#pragma unroll
					for (int i = 0; i < kPipe; ++i)
						if ((uint32_t)i < h) // unclean windows read counter 0 (unused) so that the loads stay branch-free
							vals[w][i] = C::load(a.filter, ok ? reduce_mod<POW2>(wh.at(i), a.mod) : 0);
				} else {
					window(w, ok, [&](auto&& g) {
						for (uint32_t i = 0; i < h; ++i)
							g(reduce_mod<POW2>(wh.at(i), a.mod));
					});
				}
			});
		}

		if (OP == W_QUERY && piped) {
#pragma unroll
			for (int w = 0; w < kW; ++w) {
				const bool ok = (valid_mask >> w) & 1u;
				V mn = C::kMax;
#pragma unroll
				for (int i = 0; i < kPipe; ++i)
					if ((uint32_t)i < h)
						mn = vals[w][i] < mn ? vals[w][i] : mn;
				hit_mask |= (uint32_t)(ok && mn >= (V)a.threshold) << w;
				const uint64_t gp = g0 + tid * kW + w;
				if (a.min_out && gp < a.len)
					wide_store<BYTES>(a.min_out, gp, ok ? mn : (V)0);
			}
		}

		// ---- results ----
		const uint64_t ob = (g0 >> 3) + tid;
		if (OP == W_QUERY && a.hit_bits && ob < out_bytes)
			a.hit_bits[ob] = (uint8_t)hit_mask;
		if (a.valid_bits && ob < out_bytes)
			a.valid_bits[ob] = (uint8_t)valid_mask;
		my_valid += __popc(valid_mask);
		my_hit += __popc(hit_mask);
	}

	if (a.counts) {
		const uint32_t wv = wave_sum(my_valid), wh = wave_sum(my_hit);
		if ((tid & 63) == 0) {
			atomicAdd(&sh.cnt_valid, (unsigned long long)wv);
			atomicAdd(&sh.cnt_hit, (unsigned long long)wh);
		}
		__syncthreads();
		if (tid == 0) {
			atomicAdd(reinterpret_cast<unsigned long long*>(a.counts), sh.cnt_valid);
			atomicAdd(reinterpret_cast<unsigned long long*>(a.counts) + 1, sh.cnt_hit);
		}
	}
}

template <int OP, int BYTES>
static hipError_t wide_launch_one(const SeqArgs& a, hipStream_t s, dim3 grid, size_t dyn)
{
	const bool pow2 = a.mod.pow2 != 0;
	const bool spaced = a.hp.n_seeds > 0;
#define BTLBF_WIDE_LAUNCH(P, S)                                                                                \
	do {                                                                                                       \
		if (dyn > 48 * 1024) {                                                                                 \
			hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&wide_seq_kernel<OP, BYTES, P, S>), \
			                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);           \
			if (e != hipSuccess)                                                                               \
				return e;                                                                                      \
		}                                                                                                      \
		hipLaunchKernelGGL((wide_seq_kernel<OP, BYTES, P, S>), grid, dim3(kWideThreads), dyn, s, a);           \
	} while (0)
	if (pow2 && !spaced)
		BTLBF_WIDE_LAUNCH(true, false);
	else if (!pow2 && !spaced)
		BTLBF_WIDE_LAUNCH(false, false);
	else if (pow2 && spaced)
		BTLBF_WIDE_LAUNCH(true, true);
	else
		BTLBF_WIDE_LAUNCH(false, true);
#undef BTLBF_WIDE_LAUNCH
	return hipGetLastError();
}

template <int BYTES>
static hipError_t wide_launch_op(int op, const SeqArgs& a, hipStream_t s, dim3 grid, size_t dyn)
{
	switch (op) {
	case W_QUERY: return wide_launch_one<W_QUERY, BYTES>(a, s, grid, dyn);
	case W_INC_ALL: return wide_launch_one<W_INC_ALL, BYTES>(a, s, grid, dyn);
	case W_INC_MIN: return wide_launch_one<W_INC_MIN, BYTES>(a, s, grid, dyn);
	default: return hipErrorInvalidValue;
	}
}

// the whole buffer in one launch: a few workgroups per CU, each walking a contiguous run of tiles (launch_seq_op's grid)
hipError_t launch_wide_seq_op(int op, int bytes, const SeqArgs& a_in, hipStream_t s)
{
	SeqArgs a = a_in;
	if (a.len == 0)
		return hipSuccess;
	a.first_tile = 0;
	a.n_tiles = (a.len + kWideTile - 1) / kWideTile;
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
	static_assert(kWideTile == (int)kSeqTileWindows, "seq_lds_dyn counts this kernel's tile");
	if (!seq_lds_fits(a.hp)) // (build_spaced refuses such seeds with a message; nothing is launched or configured here)
		return hipErrorInvalidValue;
	const size_t dyn = seq_lds_dyn(a.hp);
	const dim3 grid((unsigned)blocks);
	switch (bytes) {
	case 2: return wide_launch_op<2>(op, a, s, grid, dyn);
	case 4: return wide_launch_op<4>(op, a, s, grid, dyn);
	case 8: return wide_launch_op<8>(op, a, s, grid, dyn);
	default: return hipErrorInvalidValue;
	}
}

// ---- precomputed hash rows (CountingBloomFilter insert / incrementAll / minCount / contains / insertAndCheck) ---------
// op is a HashOp of the counting flavours; out: H_CBF_MIN one counter-wide element per row, else one byte per row
template <int BYTES, bool POW2>
__device__ __forceinline__ void wide_row_op(int op, void* filter, const ModParams& mod, uint32_t h, uint32_t threshold,
                                            const uint64_t* row, typename WideCtr<BYTES>::V* out)
{
	using C = WideCtr<BYTES>;
	using V = typename C::V;
	if (op == H_CBF_INC_ALL) {
		for (uint32_t i = 0; i < h; ++i)
			C::inc_sat(filter, reduce_mod<POW2>(row[i], mod));
		return;
	}
	if (op != H_CBF_INC_MIN) {
		V mn = C::kMax;
		for (uint32_t i = 0; i < h; ++i) {
			const V v = C::read_fresh(filter, reduce_mod<POW2>(row[i], mod));
			mn = v < mn ? v : mn;
		}
		*out = op == H_CBF_MIN ? mn : (V)(mn >= (V)threshold);
		if (op != H_CBF_INSERT_CHECK)
			return;
	}
	wide_increment_min<BYTES>(filter, [&](auto&& g) {
		for (uint32_t i = 0; i < h; ++i)
			g(reduce_mod<POW2>(row[i], mod));
	});
}

template <int BYTES>
__device__ __forceinline__ void wide_row_store(int op, void* out, uint64_t r, typename WideCtr<BYTES>::V v)
{
	if (!out)
		return;
	if (op == H_CBF_MIN)
		wide_store<BYTES>(out, r, v);
	else
		static_cast<uint8_t*>(out)[r] = (uint8_t)v;
}

// one lane per hash row; rows whose row_valid byte is 0 are skipped (out = 0)
template <int BYTES, bool POW2>
__global__ __launch_bounds__(256) void wide_rows_kernel(int op, void* filter, ModParams mod, uint32_t h, uint32_t threshold,
                                                        const uint64_t* hashes, uint64_t n, const uint8_t* row_valid,
                                                        void* out)
{
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
		typename WideCtr<BYTES>::V o = 0;
		if (!row_valid || row_valid[r])
			wide_row_op<BYTES, POW2>(op, filter, mod, h, threshold, hashes + r * h, &o);
		wide_row_store<BYTES>(op, out, r, o);
	}
}

// strict row order on one lane (the reference's loop, bit for bit); valid_bits: one bit per row, row_valid: one byte
template <int BYTES, bool POW2>
__global__ void wide_rows_serial_kernel(int op, void* filter, ModParams mod, uint32_t h, uint32_t threshold,
                                        const uint64_t* hashes, uint64_t n, const uint8_t* valid_bits,
                                        const uint8_t* row_valid, void* out)
{
	if (blockIdx.x != 0 || threadIdx.x != 0)
		return;
	for (uint64_t r = 0; r < n; ++r) {
		if (valid_bits && !((valid_bits[r >> 3] >> (r & 7)) & 1))
			continue;
		typename WideCtr<BYTES>::V o = 0;
		if (!row_valid || row_valid[r])
			wide_row_op<BYTES, POW2>(op, filter, mod, h, threshold, hashes + r * h, &o);
		wide_row_store<BYTES>(op, out, r, o);
	}
}

template <int BYTES, bool POW2>
static hipError_t wide_rows_launch(int op, void* filter, const ModParams& mod, uint32_t h, uint32_t threshold,
                                   const uint64_t* hashes, uint64_t n, void* out, int serial, hipStream_t s,
                                   const uint8_t* valid_bits, const uint8_t* row_valid)
{
	if (serial) {
		hipLaunchKernelGGL((wide_rows_serial_kernel<BYTES, POW2>), dim3(1), dim3(64), 0, s, op, filter, mod, h, threshold,
		                   hashes, n, valid_bits, row_valid, out);
		return hipGetLastError();
	}
	uint64_t blocks = (n + 255) / 256;
	if (blocks > 2048)
		blocks = 2048;
	hipLaunchKernelGGL((wide_rows_kernel<BYTES, POW2>), dim3((unsigned)blocks), dim3(256), 0, s, op, filter, mod, h,
	                   threshold, hashes, n, row_valid, out);
	return hipGetLastError();
}

static hipError_t wide_rows_dispatch(int op, int bytes, void* filter, const ModParams& mod, uint32_t h, uint32_t threshold,
                                     const uint64_t* hashes, uint64_t n, void* out, int serial, hipStream_t s,
                                     const uint8_t* valid_bits, const uint8_t* row_valid)
{
	if (n == 0)
		return hipSuccess;
	if (op < H_CBF_INC_MIN || op > H_CBF_INSERT_CHECK)
		return hipErrorInvalidValue;
#define BTLBF_WIDE_ROWS(B)                                                                                              \
	return mod.pow2 ? wide_rows_launch<B, true>(op, filter, mod, h, threshold, hashes, n, out, serial, s, valid_bits,  \
	                                            row_valid)                                                             \
	                : wide_rows_launch<B, false>(op, filter, mod, h, threshold, hashes, n, out, serial, s, valid_bits, \
	                                             row_valid)
	switch (bytes) {
	case 2: BTLBF_WIDE_ROWS(2);
	case 4: BTLBF_WIDE_ROWS(4);
	case 8: BTLBF_WIDE_ROWS(8);
	default: return hipErrorInvalidValue;
	}
#undef BTLBF_WIDE_ROWS
}

hipError_t launch_wide_hash_op(int op, int bytes, void* filter, const ModParams& mod, uint32_t h, uint32_t threshold,
                               const uint64_t* hashes, uint64_t n, void* out, int serial, hipStream_t s,
                               const uint8_t* row_valid)
{
	return wide_rows_dispatch(op, bytes, filter, mod, h, threshold, hashes, n, out, serial, s, nullptr, row_valid);
}

// serial-order update over the dense hash rows of a sequence buffer (row p = window p; unclean windows are skipped
// through valid_bits): the wide counterpart of launch_serial_seq_update
hipError_t launch_wide_serial_seq_update(int bytes, const SeqArgs& a, int op, const uint64_t* hashes,
                                         const uint8_t* valid_bits, hipStream_t s)
{
	return wide_rows_dispatch(op, bytes, a.filter, a.mod, a.hp.h, a.threshold, hashes, a.len, nullptr, 1, s, valid_bits,
	                          nullptr);
}

// ---- reductions: streaming 16-byte loads, one atomic per wave (popcount_kernel / compare_kernel) ---------------------
template <int BYTES>
__device__ __forceinline__ uint64_t wide_lane(const uint32_t (&w)[4], int c)
{
	if (BYTES == 2)
		return (w[c >> 1] >> ((c & 1) * 16)) & 0xffffu;
	if (BYTES == 4)
		return w[c];
	return ((uint64_t)w[2 * c + 1] << 32) | w[2 * c];
}

// mode 1: counters != 0 (popCount, CountingBloomFilter.hpp:217-228); mode 2: counters >= threshold (:231-242)
template <int BYTES>
__global__ __launch_bounds__(256) void wide_popcount_kernel(const uint4* data, uint64_t n_vec, int mode, uint32_t threshold,
                                                            unsigned long long* out)
{
	unsigned long long acc = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint4 v = data[i];
		const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
		for (int c = 0; c < 16 / BYTES; ++c) {
			const uint64_t x = wide_lane<BYTES>(w, c);
			acc += mode == 1 ? (x != 0) : (x >= (uint64_t)threshold);
		}
	}
	for (int o = 32; o > 0; o >>= 1)
		acc += __shfl_xor(acc, o, 64);
	if ((threadIdx.x & 63) == 0 && acc)
		atomicAdd(out, acc);
}

// nbytes: a multiple of 16 (filter arrays are zero-padded to 16 bytes)
hipError_t launch_wide_popcount(const void* data, uint64_t nbytes, int bytes, int mode, uint32_t threshold,
                                unsigned long long* out, hipStream_t s)
{
	if (nbytes % 16 || (mode != 1 && mode != 2))
		return hipErrorInvalidValue;
	const uint64_t n_vec = nbytes / 16;
	if (n_vec == 0)
		return hipSuccess;
	uint64_t blocks = (n_vec + 255) / 256;
	if (blocks > 4096)
		blocks = 4096;
	const dim3 grid((unsigned)blocks);
	const uint4* d = static_cast<const uint4*>(data);
	switch (bytes) {
	case 2: hipLaunchKernelGGL(wide_popcount_kernel<2>, grid, dim3(256), 0, s, d, n_vec, mode, threshold, out); break;
	case 4: hipLaunchKernelGGL(wide_popcount_kernel<4>, grid, dim3(256), 0, s, d, n_vec, mode, threshold, out); break;
	case 8: hipLaunchKernelGGL(wide_popcount_kernel<8>, grid, dim3(256), 0, s, d, n_vec, mode, threshold, out); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

// out[0] += counters that differ, out[1] += counters with a > b, out[2] += counters with a < b
template <int BYTES>
__global__ __launch_bounds__(256) void wide_compare_kernel(const uint4* a, const uint4* b, uint64_t n_vec,
                                                           unsigned long long* out)
{
	unsigned long long gt = 0, lt = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint4 va = a[i], vb = b[i];
		const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
		for (int c = 0; c < 16 / BYTES; ++c) {
			const uint64_t ca = wide_lane<BYTES>(wa, c), cb = wide_lane<BYTES>(wb, c);
			gt += ca > cb;
			lt += ca < cb;
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

hipError_t launch_wide_compare(const void* a, const void* b, uint64_t nbytes, int bytes, unsigned long long* out3,
                               hipStream_t s)
{
	if (nbytes % 16)
		return hipErrorInvalidValue;
	const uint64_t n_vec = nbytes / 16;
	if (n_vec == 0)
		return hipSuccess;
	uint64_t blocks = (n_vec + 255) / 256;
	if (blocks > 4096)
		blocks = 4096;
	const dim3 grid((unsigned)blocks);
	const uint4 *pa = static_cast<const uint4*>(a), *pb = static_cast<const uint4*>(b);
	switch (bytes) {
	case 2: hipLaunchKernelGGL(wide_compare_kernel<2>, grid, dim3(256), 0, s, pa, pb, n_vec, out3); break;
	case 4: hipLaunchKernelGGL(wide_compare_kernel<4>, grid, dim3(256), 0, s, pa, pb, n_vec, out3); break;
	case 8: hipLaunchKernelGGL(wide_compare_kernel<8>, grid, dim3(256), 0, s, pa, pb, n_vec, out3); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

} // namespace btlbf
