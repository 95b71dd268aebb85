// csrc/mibf_build_kernels.hip -- the two device helpers of the miBF builder (host_mibf_build.cpp).  Both sit next to a
// parser that delivers a few GB/s, so they are kept plain.
//   count_windows_kernel  : {windows, clean windows} of the sequences of a buffer, without hashing.  A window is k bytes
//                           inside one sequence; it is clean when base_entry (seq_core.hpp: the table every hash kernel
//                           stages its tiles through) accepts each of them.  For byte p let r(p) be the first byte of the
//                           run of accepted bytes of p's sequence that ends at p (p + 1 when p itself is refused), and
//                           s(p) the first byte of p's sequence: the window that ENDS at p exists iff s(p) <= p - k + 1
//                           and is clean iff r(p) <= p - k + 1.  Both are running maxima over the bytes up to p -- of
//                           q + 1 at a refused byte and q at the first byte of a sequence, and of q at a first byte --,
//                           so a wavefront takes 64 consecutive bytes per step, a byte per lane (coalesced whatever
//                           the buffer's alignment), carries the two maxima across its lanes with a wave scan and
//                           across steps in a register.  A wavefront owns chunks of kChunk bytes and starts k - 1
//                           bytes before each: no window that ends in the chunk begins earlier, so nothing crosses
//                           between wavefronts.  Ragged layout: the first bytes of sequences are found from starts[]
//                           with a cursor per wavefront (a binary search per chunk, then 64 offsets per step, loaded
//                           coalesced and turned into a lane mask).  Counts per lane, wave and block reduction, one
//                           64-bit atomic per block and count.
//   mibf_fill_ids_kernel  : the ids of a batch's sequences: first + i (an id per record) or first (the file's id).
#include "seq_core.hpp"

#include <algorithm>

namespace btlbf {

static constexpr uint32_t kCountChunk = 8192; // bytes of a wavefront's chunk: 128 steps + the k - 1 bytes before it

__device__ __forceinline__ uint32_t wave_scan_max(uint32_t v, uint32_t lane)
{
	for (uint32_t o = 1; o < 64; o <<= 1) {
		const uint32_t t = __shfl_up(v, o, 64);
		if (lane >= o)
			v = v > t ? v : t;
	}
	return v;
}

__device__ __forceinline__ unsigned long long wave_or64(unsigned long long v)
{
	for (int o = 32; o > 0; o >>= 1)
		v |= __shfl_xor(v, o, 64);
	return v;
}

__global__ __launch_bounds__(256) void count_windows_kernel(const uint8_t* __restrict__ seq, uint64_t len,
                                                            LayoutParams lay, uint32_t k, unsigned long long* out2)
{
	__shared__ unsigned long long tot[2][4];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t n_chunks = (len + kCountChunk - 1) / kCountChunk;
	const uint64_t n_waves = (uint64_t)gridDim.x * 4;
	unsigned long long windows = 0, clean = 0; // of this lane
	for (uint64_t c = (uint64_t)blockIdx.x * 4 + wave; c < n_chunks; c += n_waves) {
		const uint64_t c0 = c * kCountChunk, c1 = c0 + kCountChunk < len ? c0 + kCountChunk : len;
		const uint64_t base = c0 >= k - 1 ? c0 - (k - 1) : 0; // positions below are relative to it, and fit 32 bits
		// ragged: the first offset at or after base (offsets 1 .. n_seqs - 1 begin a sequence inside the buffer; offset 0
		// is the buffer's first byte, where every chunk that reaches it starts afresh anyway)
		uint64_t cur = 0;
		if (lay.starts) {
			uint64_t lo = 0, hi = lay.n_seqs;
			while (lo < hi) {
				const uint64_t mid = lo + (hi - lo) / 2;
				if (lay.starts[mid] < base)
					lo = mid + 1;
				else
					hi = mid;
			}
			cur = lo;
		}
		// uniform: byte base + rel is the first of a read iff rel % read_len equals this
		const uint32_t first_rem = lay.read_len ? (uint32_t)((lay.read_len - base % lay.read_len) % lay.read_len) : 0;
		uint32_t run_c = 0, seq_c = 0; // the carried maxima: the run and the sequence begin at base unless a byte says otherwise
		for (uint64_t g = base; g < c1; g += 64) {
			const uint64_t p = g + lane;
			const uint32_t rel = (uint32_t)(p - base);
			const bool in = p < c1;
			bool first = false;
			if (lay.starts) {
				unsigned long long mask = 0;
				for (;;) { // 64 offsets per round: one round unless the step holds more than 63 sequences (empty ones)
					const uint64_t i = cur + lane;
					const uint64_t v = i < lay.n_seqs ? lay.starts[i] : ~0ull;
					const bool here = v < g + 64;
					const unsigned long long any = __ballot(here);
					if (any == 0)
						break;
					mask |= wave_or64(here && v >= g ? 1ull << (v - g) : 0ull);
					cur += __popcll(any);
					if (any != ~0ull)
						break;
				}
				first = (mask >> lane) & 1;
			} else if (lay.read_len) {
				first = rel % lay.read_len == first_rem;
			}
			const bool good = in && base_entry(seq[p]) != 0;
			uint32_t run = wave_scan_max(!in ? 0u : !good ? rel + 1 : first ? rel : 0u, lane);
			uint32_t sq = wave_scan_max(in && first ? rel : 0u, lane);
			run = run > run_c ? run : run_c;
			sq = sq > seq_c ? sq : seq_c;
			run_c = __shfl(run, 63, 64);
			seq_c = __shfl(sq, 63, 64);
			if (in && p >= c0 && rel + 1 >= k) { // the window that ends at p begins at rel + 1 - k
				windows += sq <= rel + 1 - k;
				clean += run <= rel + 1 - k;
			}
		}
	}
	unsigned long long w = windows, cl = clean;
	for (int o = 32; o > 0; o >>= 1) {
		w += __shfl_xor(w, o, 64);
		cl += __shfl_xor(cl, o, 64);
	}
	if (lane == 0) {
		tot[0][wave] = w;
		tot[1][wave] = cl;
	}
	__syncthreads();
	if (threadIdx.x < 2) {
		const unsigned long long t = tot[threadIdx.x][0] + tot[threadIdx.x][1] + tot[threadIdx.x][2] + tot[threadIdx.x][3];
		if (t)
			atomicAdd(out2 + threadIdx.x, t);
	}
}

hipError_t launch_count_windows(const uint8_t* seq, uint64_t len, const LayoutParams& lay, uint32_t k,
                                unsigned long long* out2, hipStream_t s)
{
	if (len < k || k == 0)
		return hipSuccess;
	const uint64_t n_chunks = (len + kCountChunk - 1) / kCountChunk;
	const uint64_t blocks = std::min<uint64_t>((n_chunks + 3) / 4, 4096);
	hipLaunchKernelGGL(count_windows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, seq, len, lay, k, out2);
	return hipGetLastError();
}

__global__ __launch_bounds__(256) void mibf_fill_ids_kernel(uint32_t* ids, uint64_t n, uint32_t first, uint32_t step)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
		ids[i] = first + (uint32_t)i * step;
}

hipError_t launch_mibf_fill_ids(uint32_t* ids, uint64_t n, uint32_t first, uint32_t step, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 4096);
	hipLaunchKernelGGL(mibf_fill_ids_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ids, n, first, step);
	return hipGetLastError();
}

} // namespace btlbf
