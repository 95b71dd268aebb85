// csrc/mibf_kernels.hip -- the multi-index Bloom filter (miBF) stages 3 and 4: the ID array over the rank structure.
//
// The reference's miBF (MIBloomFilter.hpp, MIBFConstructSupport.hpp, MIBFQuerySupport.hpp) addresses an array of
// IDs of type T (uint16_t / uint32_t here) with rank(hash % size) over its stage-1 bit vector; the rank records are
// the interleaved 72-byte records of aux_kernels.hip (sdsl::bit_vector_il<512> layout).  Kernels:
//   mibf_seq_kernel<MIBF_EMIT>  : window hashing (seq_core.hpp) fused with the rank of every hash value; emits one
//                                 (rank << seq_bits | sequence, hash) pair per hash of a clean window (insertMIBF)
//   mibf_insert_apply_kernel    : after a radix sort by (rank, sequence): one lane per rank segment walks the
//                                 sequences in order, each sequence's distinct hash values in ascending order, and
//                                 runs the reservoir step (MIBFConstructSupport.hpp:109-130); data / counts are
//                                 written once per touched rank, with no atomics
//   mibf_seq_kernel<MIBF_DECIDE>: insertSaturation's decision (MIBFConstructSupport.hpp:166-213) of every window
//                                 against the arrays as they stood at the start of the call; decisions are compacted
//   mibf_mutate_apply_kernel    : after a sort of the mutations by rank: counts += choosers, the last chooser's id by
//                                 setData's rule (MIBloomFilter.hpp:625-634)
//   mibf_saturate_kernel        : saturate() (MIBloomFilter.hpp:440-446): 32-bit atomic OR of the shifted mask
//   mibf_serial_saturate_kernel : the reference's single-threaded loop, one lane over precomputed hash rows
//   mibf_seq_kernel<MIBF_QUERY> : getMatchSignature (MIBFQuerySupport.hpp:158-217) over atRank
//                                 (MIBloomFilter.hpp:478-515): raw T values, match bits, counts
//   mibf_stats_kernel / mibf_hist_kernel: getPopNonZero / getPopSaturated / getIDCounts (MIBloomFilter.hpp:539-620)
#include "seq_core.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <type_traits>

namespace btlbf {

static constexpr int kMThreads = 256;
static constexpr int kMTile = kMThreads * kW;

// rank(p) = set bits before position p over the interleaved records (aux_kernels.hip rank_query_kernel); bit = bit p
__device__ __forceinline__ uint64_t mibf_rank(const uint64_t* il, uint64_t p, uint32_t& bit)
{
	const uint64_t* rec = il + (p >> 9) * 9;
	const uint32_t wq = (uint32_t)(p >> 6) & 7, sh = (uint32_t)p & 63;
	uint64_t r = rec[0];
#pragma unroll
	for (uint32_t q = 0; q < 7; ++q)
		if (q < wq)
			r += __popcll(rec[1 + q]);
	const uint64_t w = rec[1 + wq];
	bit = (uint32_t)(w >> sh) & 1u;
	return r + __popcll(w & ((1ull << sh) - 1));
}

// index of the sequence holding byte gp of the batch: uniform reads, ragged starts[] (binary search, cached per lane
// in [lo, hi)), or one sequence for the whole buffer
struct SeqCursor {
	uint64_t s = 0, lo = 1, hi = 0;
	__device__ __forceinline__ uint64_t at(const LayoutParams& lay, uint64_t gp)
	{
		if (lay.read_len)
			return gp / lay.read_len;
		if (!lay.starts)
			return 0;
		if (gp >= lo && gp < hi)
			return s;
		uint64_t a = 0, b = lay.n_seqs; // largest a with starts[a] <= gp
		while (b - a > 1) {
			const uint64_t m = (a + b) >> 1;
			if (lay.starts[m] <= gp)
				a = m;
			else
				b = m;
		}
		s = a;
		lo = lay.starts[a];
		hi = lay.starts[a + 1];
		return s;
	}
};

template <class T>
struct MibfMask {
	static constexpr T mask = (T)((T)1 << (sizeof(T) * 8 - 1));
	static constexpr T anti = (T)~mask;
};

// setData (MIBloomFilter.hpp:625-634): the id keeps the saturation bit iff the old value is above the mask
template <class T>
__device__ __forceinline__ T mibf_set_data(T old, T id)
{
	return old > MibfMask<T>::mask ? (T)(id | MibfMask<T>::mask) : id;
}

// hash % size (a uniform branch: the miBF kernels are not instantiated per modulus kind)
__device__ __forceinline__ uint64_t mibf_reduce(uint64_t v, const ModParams& m)
{
	return m.pow2 ? (v & m.mask) : reduce_mod<false>(v, m);
}

// HS = 0: plain ntHash (ntHashIterator); HS = 1..8: that many spaced seeds with h2 = 1 (stHashIterator), the hash
// values held in registers (seq_core.hpp's union-list walk: part_supported)
template <int OP, int HS, class T>
__global__ __launch_bounds__(kMThreads) void mibf_seq_kernel(const MibfArgs a)
{
	constexpr bool SPACED = HS > 0;
	extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
	__shared__ SeqShared sh;
	__shared__ unsigned long long wg_cnt[4];

	const uint32_t tid = threadIdx.x;
	const uint32_t k = a.hp.k, h = a.hp.h;
	const uint32_t tile_cap = seq_tile_cap(kMTile, k);
	uint8_t* tile = dyn;
	uint8_t* spaced_lds = dyn + tile_cap;
	if (tid < 4)
		wg_cnt[tid] = 0;
	seq_setup_tables<kMThreads, SPACED>(sh, a.hp, spaced_lds);

	const uint64_t t_begin = (uint64_t)blockIdx.x * a.tiles_per_block;
	uint64_t t_end = t_begin + a.tiles_per_block;
	const uint64_t n_tiles = (a.len + kMTile - 1) / kMTile;
	if (t_end > n_tiles)
		t_end = n_tiles;
	const uint32_t L = a.layout.starts ? 0 : a.layout.read_len;
	uint32_t tile_off = 0;
	if (L && t_begin < t_end)
		tile_off = (uint32_t)((t_begin * (uint64_t)kMTile) % L);
	const uint32_t tile_step = L ? (uint32_t)(kMTile % L) : 0;
	const uint64_t out_bytes = ((a.len + 63) / 64) * 8;
	const T* data = static_cast<const T*>(a.data);
	SeqCursor cur;
	uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0; // EMIT/QUERY: clean, matched; DECIDE: clean, found, mutated, saturated

	for (uint64_t t = t_begin; t < t_end; ++t) {
		const uint64_t g0 = t * (uint64_t)kMTile;
		const uint32_t mis = seq_stage_tile<kMThreads>(tile, tile_cap, sh, a.seq, a.len, a.layout, k, g0, tile_off);
		tile_off = seq_next_tile_off(tile_off, tile_step, L);
		uint32_t valid_mask = 0, hit_mask = 0;

		seq_lane_windows<SPACED, kW, HS>(tile, sh, a.hp, spaced_lds, tid * kW + mis, [&](int w, bool ok, const WinHash<SPACED>& wh) {
			const uint64_t gp = g0 + tid * kW + w;
			if (gp >= a.len)
				return;
			valid_mask |= (uint32_t)ok << w;
			c0 += ok;
			if (OP == MIBF_EMIT) {
				// insertMIBF's value set: every hash of every clean window, keyed by (rank, sequence)
				const uint64_t sk = ok ? cur.at(a.layout, gp) : 0;
#pragma unroll
				for (uint32_t i = 0; i < kMibfMaxHash; ++i) {
					if (i >= h)
						break;
					uint64_t key = ~0ull, v = 0;
					if (ok) {
						v = wh.at(i);
						uint32_t bit;
						key = mibf_rank(a.il, mibf_reduce(v, a.mod), bit) << a.seq_bits | sk;
					}
					a.keys[gp * h + i] = key;
					a.vals[gp * h + i] = v;
				}
			} else if (OP == MIBF_DECIDE) {
				if (!ok)
					return;
				// setSatIfMissing (MIBFConstructSupport.hpp:166-213) against the snapshot
				const T id = (T)a.ids[a.seq0 + cur.at(a.layout, gp)];
				uint64_t rk[kMibfMaxHash];
				T x[kMibfMaxHash];
				bool found = false;
#pragma unroll
				for (uint32_t i = 0; i < kMibfMaxHash; ++i) {
					if (i < h) {
						uint32_t bit;
						rk[i] = mibf_rank(a.il, mibf_reduce(wh.at(i), a.mod), bit);
						x[i] = (T)(data[rk[i]] & MibfMask<T>::anti);
						found |= x[i] == id;
					}
				}
				if (found) {
					++c1;
					return;
				}
				// replacementIDs = {0} + every value seen before at a lower index (seenSet starts with h zeros), so
				// position i qualifies iff x[i] == 0 or x[i] occurs twice; the largest count by strict > from 0 wins
				T best = 0;
				uint64_t pos = ~0ull;
#pragma unroll
				for (uint32_t i = 0; i < kMibfMaxHash; ++i) {
					if (i < h) {
						bool rep = x[i] == 0;
#pragma unroll
						for (uint32_t j = 0; j < kMibfMaxHash; ++j)
							rep |= j < h && j != i && x[j] == x[i];
						if (rep) {
							const T c = a.counts_t ? static_cast<const T*>(a.counts_t)[rk[i]] : 0;
							if (best < c) {
								best = c;
								pos = rk[i];
							}
						}
					}
				}
				if (pos != ~0ull) {
					++c2;
					const unsigned long long slot = atomicAdd(a.n_out, 1ull);
					if (slot < a.cap_mut) { // (rank, chooser's window); the apply step finds the chooser's id again
						a.keys[slot] = pos;
						a.vals[slot] = gp;
					}
				} else {
					++c3;
					const unsigned long long slot = atomicAdd(a.n_out + 1, (unsigned long long)h);
					for (uint32_t i = 0; i < h; ++i)
						if (slot + i < a.cap_sat)
							a.sat[slot + i] = rk[i];
				}
			} else { // MIBF_QUERY
				if (!ok) {
					for (uint32_t i = 0; i < h; ++i)
						static_cast<T*>(a.values)[gp * h + i] = 0;
					if (a.hit_masks)
						a.hit_masks[gp] = 0;
					return;
				}
				// atRank (MIBloomFilter.hpp:478-515) + getMatchSignature (MIBFQuerySupport.hpp:158-217)
				uint64_t rk[kMibfMaxHash];
				uint32_t hits = 0, misses = 0;
#pragma unroll
				for (uint32_t i = 0; i < kMibfMaxHash; ++i) {
					if (i < h) {
						uint32_t bit;
						rk[i] = mibf_rank(a.il, mibf_reduce(wh.at(i), a.mod), bit);
						hits |= bit << i;
						misses += bit ^ 1u;
					}
				}
				const bool match = SPACED ? misses <= a.max_miss : misses == 0;
				T vals[kMibfMaxHash];
#pragma unroll
				for (uint32_t i = 0; i < kMibfMaxHash; ++i)
					if (i < h)
						vals[i] = match && ((hits >> i) & 1u) ? data[rk[i]] : (T)0;
#pragma unroll
				for (uint32_t i = 0; i < kMibfMaxHash; ++i)
					if (i < h)
						static_cast<T*>(a.values)[gp * h + i] = vals[i];
				if (a.hit_masks)
					a.hit_masks[gp] = match ? (uint8_t)hits : (uint8_t)0;
				hit_mask |= (uint32_t)match << w;
				c1 += match;
			}
		});

		if (OP == MIBF_QUERY) {
			const uint64_t ob = (g0 >> 3) + tid;
			if (ob < out_bytes) {
				if (a.hit_bits)
					a.hit_bits[ob] = (uint8_t)hit_mask;
				if (a.valid_bits)
					a.valid_bits[ob] = (uint8_t)valid_mask;
			}
		}
	}

	if (a.stat) {
		const uint32_t v0 = wave_sum(c0), v1 = wave_sum(c1), v2 = wave_sum(c2), v3 = wave_sum(c3);
		__syncthreads();
		if ((tid & 63) == 0) {
			atomicAdd(&wg_cnt[0], (unsigned long long)v0);
			atomicAdd(&wg_cnt[1], (unsigned long long)v1);
			atomicAdd(&wg_cnt[2], (unsigned long long)v2);
			atomicAdd(&wg_cnt[3], (unsigned long long)v3);
		}
		__syncthreads();
		if (tid < 4 && wg_cnt[tid])
			atomicAdd(a.stat + tid, wg_cnt[tid]);
	}
}

// insertMIBF (MIBFConstructSupport.hpp:109-130) of one batch, after the sort by key = rank << seq_bits | sequence:
// the lane at the head of a rank segment walks it -- sequences in order, each sequence's hash values sorted in place
// (ascending; a value seen twice counts once) -- and writes the rank's count and ID once.  Keys ~0 (windows that are not
// clean) sort behind every real key.
template <class T>
__global__ __launch_bounds__(256) void mibf_insert_apply_kernel(const uint64_t* keys, uint64_t* vals, uint64_t n,
                                                                uint32_t seq_bits, const uint32_t* ids, uint64_t seq0,
                                                                T* data, T* counts)
{
	const uint64_t smask = (1ull << seq_bits) - 1;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t key = keys[i];
		const uint64_t r = key >> seq_bits;
		if (key == ~0ull || (i > 0 && keys[i - 1] >> seq_bits == r))
			continue;
		T c = counts[r], d = data[r];
		uint64_t j = i;
		while (j < n && keys[j] != ~0ull && keys[j] >> seq_bits == r) {
			const uint64_t kj = keys[j];
			uint64_t e = j + 1;
			while (e < n && keys[e] == kj)
				++e;
			for (uint64_t q = j + 1; q < e; ++q) { // insertion sort of the group's hash values (groups are short)
				const uint64_t v = vals[q];
				uint64_t p = q;
				while (p > j && vals[p - 1] > v) {
					vals[p] = vals[p - 1];
					--p;
				}
				vals[p] = v;
			}
			const T id = (T)ids[seq0 + (kj & smask)];
			for (uint64_t q = j; q < e; ++q) {
				const uint64_t v = vals[q];
				if (q > j && v == vals[q - 1])
					continue;
				c = (T)(c + 1);
				const T x = (T)(v ^ (uint64_t)id); // std::hash<T> of the seed converted to T: the identity
				if (c != 0 && (T)(x % c) == (T)(c - 1)) // c == 0 (wrapped counter) is UB in the reference: no replacement
					d = mibf_set_data<T>(d, id);
			}
			j = e;
		}
		counts[r] = c;
		data[r] = d;
	}
}

// the mutations of a parallel insertSaturation, sorted by rank (payload = the chooser's window): counts += choosers
// (T wrap), the ID of the last chooser in window order by setData's rule against the snapshot value
template <class T>
__global__ __launch_bounds__(256) void mibf_mutate_apply_kernel(const uint64_t* keys, const uint64_t* vals, uint64_t n,
                                                                const LayoutParams lay, const uint32_t* ids, T* data,
                                                                T* counts)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t r = keys[i];
		if (i > 0 && keys[i - 1] == r)
			continue;
		uint64_t last = vals[i], m = 0;
		for (uint64_t j = i; j < n && keys[j] == r; ++j, ++m)
			last = vals[j] > last ? vals[j] : last;
		SeqCursor cur;
		const T id = (T)ids[cur.at(lay, last)];
		counts[r] = (T)(counts[r] + (T)m);
		data[r] = mibf_set_data<T>(data[r], id);
	}
}

// saturate (MIBloomFilter.hpp:440-446): OR the mask into the ID at each rank, as a 32-bit atomic on the word holding it
template <class T>
__global__ __launch_bounds__(256) void mibf_saturate_kernel(const uint64_t* ranks, uint64_t n, uint32_t* words)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t r = ranks[i];
		if (sizeof(T) == 4)
			atomicOr(words + r, (uint32_t)MibfMask<T>::mask);
		else
			atomicOr(words + (r >> 1), (uint32_t)MibfMask<T>::mask << ((r & 1) * 16));
	}
}

// BTLBF_ORDER_SERIAL insertSaturation: the reference's single-threaded loop over the windows in buffer order, on hash
// rows (len x h, window gp at row gp) and their clean bits.  One lane: for parity and small inputs.
template <class T>
__global__ __launch_bounds__(64) void mibf_serial_saturate_kernel(const uint64_t* rows, const uint64_t* valid, uint64_t len,
                                                                  uint32_t h, const ModParams mod, const uint64_t* il,
                                                                  const LayoutParams lay, const uint32_t* ids,
                                                                  uint64_t seq0, T* data, T* counts,
                                                                  unsigned long long* stat)
{
	if (threadIdx.x != 0 || blockIdx.x != 0)
		return;
	SeqCursor cur;
	unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
	for (uint64_t gp = 0; gp < len; ++gp) {
		if (!((valid[gp >> 6] >> (gp & 63)) & 1))
			continue;
		++c0;
		const T id = (T)ids[seq0 + cur.at(lay, gp)];
		uint64_t rk[kMibfMaxHash];
		T x[kMibfMaxHash];
		bool found = false;
		for (uint32_t i = 0; i < h; ++i) {
			uint32_t bit;
			const uint64_t hv = rows[gp * h + i];
			rk[i] = mibf_rank(il, mibf_reduce(hv, mod), bit);
			x[i] = (T)(data[rk[i]] & MibfMask<T>::anti);
			found |= x[i] == id;
		}
		if (found) {
			++c1;
			continue;
		}
		T best = 0;
		uint64_t pos = ~0ull;
		for (uint32_t i = 0; i < h; ++i) {
			bool rep = x[i] == 0;
			for (uint32_t j = 0; j < i; ++j)
				rep |= x[j] == x[i];
			for (uint32_t j = i + 1; j < h; ++j)
				rep |= x[j] == x[i];
			if (rep && best < counts[rk[i]]) {
				best = counts[rk[i]];
				pos = rk[i];
			}
		}
		if (pos != ~0ull) {
			++c2;
			data[pos] = mibf_set_data<T>(data[pos], id);
			counts[pos] = (T)(counts[pos] + 1);
		} else {
			++c3;
			for (uint32_t i = 0; i < h; ++i)
				data[rk[i]] = (T)(data[rk[i]] | MibfMask<T>::mask);
		}
	}
	stat[0] += c0;
	stat[1] += c1;
	stat[2] += c2;
	stat[3] += c3;
}

// getPopNonZero / getPopSaturated (MIBloomFilter.hpp:571-620): out[0] += nonzero, out[1] += above the mask
template <class T>
__global__ __launch_bounds__(256) void mibf_stats_kernel(const T* data, uint64_t n, unsigned long long* out)
{
	uint32_t nz = 0, sat = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const T v = data[i];
		nz += v != 0;
		sat += v > MibfMask<T>::mask;
	}
	nz = wave_sum(nz);
	sat = wave_sum(sat);
	if ((threadIdx.x & 63) == 0) {
		if (nz)
			atomicAdd(out, (unsigned long long)nz);
		if (sat)
			atomicAdd(out + 1, (unsigned long long)sat);
	}
}

// getIDCounts (MIBloomFilter.hpp:539-551): bin = v & antiMask when v > mask, else v; bins >= n_bins are not counted
// (the reference would index past its vector).  Workgroup-private bins in LDS when they fit.
static constexpr uint32_t kHistLds = 8192;
template <class T>
__global__ __launch_bounds__(256) void mibf_hist_kernel(const T* data, uint64_t n, uint64_t n_bins,
                                                        unsigned long long* bins)
{
	__shared__ uint32_t lb[kHistLds];
	const bool local = n_bins <= kHistLds;
	if (local)
		for (uint32_t b = threadIdx.x; b < n_bins; b += blockDim.x)
			lb[b] = 0;
	__syncthreads();
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const T v = data[i];
		const uint64_t b = v > MibfMask<T>::mask ? (uint64_t)(T)(v & MibfMask<T>::anti) : (uint64_t)v;
		if (b < n_bins) {
			if (local)
				atomicAdd(lb + b, 1u);
			else
				atomicAdd(bins + b, 1ull);
		}
	}
	__syncthreads();
	if (local)
		for (uint32_t b = threadIdx.x; b < n_bins; b += blockDim.x)
			if (lb[b])
				atomicAdd(bins + b, (unsigned long long)lb[b]);
}

// ---- launchers ---------------------------------------------------------------------------------------------------

hipError_t launch_mibf_seq(MibfOp op, int id_bytes, const MibfArgs& a_in, hipStream_t s)
{
	MibfArgs a = a_in;
	if (a.len == 0)
		return hipSuccess;
	const uint64_t n_tiles = (a.len + kMTile - 1) / kMTile;
	int dev = 0, cus = 256;
	if (hipGetDevice(&dev) == hipSuccess) {
		int v = 0;
		if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
			cus = v;
	}
	const uint64_t max_blocks = (uint64_t)cus * 8;
	uint64_t blocks = n_tiles < max_blocks ? n_tiles : max_blocks;
	a.tiles_per_block = (n_tiles + blocks - 1) / blocks;
	blocks = (n_tiles + a.tiles_per_block - 1) / a.tiles_per_block;
	static_assert(kMTile == (int)kSeqTileWindows, "seq_lds_dyn counts this kernel's tile");
	static_assert(sizeof(SeqShared) + 4 * sizeof(unsigned long long) <= kSeqStaticLds, "kSeqStaticLds covers SeqShared and wg_cnt");
	if (!seq_lds_fits(a.hp)) // (build_spaced refuses such seeds with a message; nothing is launched or configured here)
		return hipErrorInvalidValue;
	const size_t dyn = seq_lds_dyn(a.hp);
	const int hs = a.hp.n_seeds ? (int)a.hp.h : 0;
	auto go = [&](auto kernel) -> hipError_t {
		if (dyn > 48 * 1024) {
			hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
			                                   (int)dyn);
			if (e != hipSuccess)
				return e;
		}
		hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kMThreads), dyn, s, a);
		return hipGetLastError();
	};
	auto by_hs = [&](auto op_c, auto t) -> hipError_t {
		constexpr int OP = decltype(op_c)::value;
		using T = decltype(t);
		switch (hs) {
		case 0: return go(mibf_seq_kernel<OP, 0, T>);
		case 1: return go(mibf_seq_kernel<OP, 1, T>);
		case 2: return go(mibf_seq_kernel<OP, 2, T>);
		case 3: return go(mibf_seq_kernel<OP, 3, T>);
		case 4: return go(mibf_seq_kernel<OP, 4, T>);
		case 5: return go(mibf_seq_kernel<OP, 5, T>);
		case 6: return go(mibf_seq_kernel<OP, 6, T>);
		case 7: return go(mibf_seq_kernel<OP, 7, T>);
		case 8: return go(mibf_seq_kernel<OP, 8, T>);
		default: return hipErrorInvalidValue;
		}
	};
	return mibf_by_id(id_bytes, [&](auto t) {
		switch (op) {
		case MIBF_EMIT: return by_hs(std::integral_constant<int, MIBF_EMIT>(), t);
		case MIBF_DECIDE: return by_hs(std::integral_constant<int, MIBF_DECIDE>(), t);
		case MIBF_QUERY: return by_hs(std::integral_constant<int, MIBF_QUERY>(), t);
		default: return hipErrorInvalidValue;
		}
	});
}

// sort scratch of rocPRIM's radix sort for n 64-bit key / 64-bit value pairs
hipError_t mibf_sort_temp_bytes(uint64_t n, size_t* bytes)
{
	*bytes = 0;
	return rocprim::radix_sort_pairs(nullptr, *bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
	                                 (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n, 0, 64);
}

hipError_t mibf_sort_pairs(void* temp, size_t temp_bytes, const uint64_t* k_in, uint64_t* k_out, const uint64_t* v_in,
                           uint64_t* v_out, uint64_t n, uint32_t end_bit, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	return rocprim::radix_sort_pairs(temp, temp_bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, end_bit, s);
}

// a grid-stride kernel over n items: at most max_grid workgroups of 256 lanes
template <class K, class... A>
static hipError_t launch_over(uint64_t n, uint64_t max_grid, hipStream_t s, K kernel, A... args)
{
	if (n == 0)
		return hipSuccess;
	hipLaunchKernelGGL(kernel, dim3((unsigned)std::min((n + 255) / 256, max_grid)), dim3(256), 0, s, args...);
	return hipGetLastError();
}

hipError_t launch_mibf_insert_apply(int id_bytes, const uint64_t* keys, uint64_t* vals, uint64_t n, uint32_t seq_bits,
                                    const uint32_t* ids, uint64_t seq0, void* data, void* counts, hipStream_t s)
{
	return mibf_by_id(id_bytes, [&](auto t) {
		using T = decltype(t);
		return launch_over(n, 65536, s, mibf_insert_apply_kernel<T>, keys, vals, n, seq_bits, ids, seq0, static_cast<T*>(data),
		                   static_cast<T*>(counts));
	});
}

hipError_t launch_mibf_mutate_apply(int id_bytes, const uint64_t* keys, const uint64_t* vals, uint64_t n,
                                    const LayoutParams& lay, const uint32_t* ids, void* data, void* counts, hipStream_t s)
{
	return mibf_by_id(id_bytes, [&](auto t) {
		using T = decltype(t);
		return launch_over(n, 65536, s, mibf_mutate_apply_kernel<T>, keys, vals, n, lay, ids, static_cast<T*>(data),
		                   static_cast<T*>(counts));
	});
}

hipError_t launch_mibf_saturate(int id_bytes, const uint64_t* ranks, uint64_t n, void* data, hipStream_t s)
{
	return mibf_by_id(id_bytes, [&](auto t) {
		return launch_over(n, 65536, s, mibf_saturate_kernel<decltype(t)>, ranks, n, static_cast<uint32_t*>(data));
	});
}

hipError_t launch_mibf_serial_saturate(int id_bytes, const uint64_t* rows, const uint64_t* valid, uint64_t len, uint32_t h,
                                       const ModParams& mod, const uint64_t* il, const LayoutParams& lay,
                                       const uint32_t* ids, uint64_t seq0, void* data, void* counts,
                                       unsigned long long* stat, hipStream_t s)
{
	return mibf_by_id(id_bytes, [&](auto t) {
		using T = decltype(t);
		hipLaunchKernelGGL(mibf_serial_saturate_kernel<T>, dim3(1), dim3(64), 0, s, rows, valid, len, h, mod, il, lay, ids,
		                   seq0, static_cast<T*>(data), static_cast<T*>(counts), stat);
		return hipGetLastError();
	});
}

hipError_t launch_mibf_stats(int id_bytes, const void* data, uint64_t n, unsigned long long* out2, hipStream_t s)
{
	return mibf_by_id(id_bytes, [&](auto t) {
		using T = decltype(t);
		return launch_over(n, 4096, s, mibf_stats_kernel<T>, static_cast<const T*>(data), n, out2);
	});
}

hipError_t launch_mibf_hist(int id_bytes, const void* data, uint64_t n, uint64_t n_bins, unsigned long long* bins,
                            hipStream_t s)
{
	if (n_bins == 0)
		return hipSuccess;
	return mibf_by_id(id_bytes, [&](auto t) {
		using T = decltype(t);
		return launch_over(n, 2048, s, mibf_hist_kernel<T>, static_cast<const T*>(data), n, n_bins, bins);
	});
}

} // namespace btlbf
