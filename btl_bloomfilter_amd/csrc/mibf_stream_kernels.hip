// csrc/mibf_stream_kernels.hip -- the two device helpers of the file classifier (host_mibf_fastx.cpp): both sit next to
// a classification that does h random gathers per k-mer, so they are kept plain.
//   interleave_mates_kernel : two ragged buffers (mate 1 and mate 2 of every pair) -> the interleaved buffer
//                             btlbf_mibf_classify_pairs takes.  One wavefront per pair; the output offsets are closed
//                             form (no scan): out_starts[2i] = starts1[i] + starts2[i], out_starts[2i+1] =
//                             starts1[i+1] + starts2[i].  A mate starts and lands at any byte offset, so the copy is
//                             byte per lane: 64 consecutive bytes per wave instruction coalesce whatever the alignment,
//                             and a pair moves ~300 bytes.
//   mibf_tally_kernel       : the summary of a batch of classify results added to running totals: best[id] (first record
//                             of a row), any[id] (every record of a row), six totals.  Workgroup bins in LDS up to
//                             kTallyLds ids (as mibf_hist_kernel), flushed with 64-bit atomics; global 64-bit atomics
//                             beyond that.
#include "device_utils.hpp"

#include <algorithm>

namespace btlbf {

__global__ __launch_bounds__(256) void interleave_mates_kernel(const uint8_t* __restrict__ seq1, const uint64_t* starts1,
                                                               const uint8_t* __restrict__ seq2, const uint64_t* starts2,
                                                               uint64_t n_pairs, uint8_t* __restrict__ out,
                                                               uint64_t* out_starts)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
	for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n_pairs; i += waves) {
		const uint64_t a0 = starts1[i], a1 = starts1[i + 1], b0 = starts2[i], b1 = starts2[i + 1];
		const uint64_t o1 = a0 + b0, o2 = a1 + b0;
		if (lane == 0) {
			out_starts[2 * i] = o1;
			out_starts[2 * i + 1] = o2;
			if (i + 1 == n_pairs)
				out_starts[2 * n_pairs] = a1 + b1;
		}
		if (a1 < a0 || b1 < b0)
			continue; // offsets that decrease describe no bytes (classify refuses the layout)
		for (uint64_t j = lane; j < a1 - a0; j += 64)
			out[o1 + j] = seq1[a0 + j];
		for (uint64_t j = lane; j < b1 - b0; j += 64)
			out[o2 + j] = seq2[b0 + j];
	}
}

hipError_t launch_interleave_mates(const uint8_t* seq1, const uint64_t* starts1, const uint8_t* seq2,
                                   const uint64_t* starts2, uint64_t n_pairs, uint8_t* out, uint64_t* out_starts,
                                   hipStream_t s)
{
	if (n_pairs == 0)
		return hipMemsetAsync(out_starts, 0, 8, s);
	const uint64_t blocks = std::min<uint64_t>((n_pairs + 3) / 4, 16384);
	hipLaunchKernelGGL(interleave_mates_kernel, dim3((unsigned)blocks), dim3(256), 0, s, seq1, starts1, seq2, starts2,
	                   n_pairs, out, out_starts);
	return hipGetLastError();
}

static constexpr uint32_t kTallyLds = 8192; // ids with workgroup bins: best and any, 32 bits each = 64 KiB of LDS

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}

__global__ __launch_bounds__(256) void mibf_tally_kernel(const uint32_t* hit_words, const uint32_t* n_hits,
                                                         const uint32_t* sat_count, const uint32_t* eval_count,
                                                         uint64_t n_rows, uint32_t max_results, uint64_t n_ids,
                                                         unsigned long long* best, unsigned long long* any,
                                                         unsigned long long* totals)
{
	__shared__ uint32_t lb[2 * kTallyLds]; // best, then any
	const bool local = n_ids <= kTallyLds;
	if (local)
		for (uint32_t b = threadIdx.x; b < (uint32_t)n_ids; b += blockDim.x)
			lb[b] = lb[kTallyLds + b] = 0;
	__syncthreads();
	uint32_t rows = 0, none = 0, multi = 0, trunc = 0;
	unsigned long long sat = 0, ev = 0;
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t nh = n_hits[r];
		++rows;
		none += nh == 0;
		multi += nh > 1;
		trunc += nh > max_results;
		sat += sat_count[r];
		ev += eval_count[r];
		const uint32_t w = nh < max_results ? nh : max_results;
		const uint32_t* rec = hit_words + r * max_results * 4; // btlbf_mibf_hit: 16 bytes, id in its first word
		for (uint32_t j = 0; j < w; ++j) {
			const uint64_t id = rec[j * 4];
			if (id >= n_ids)
				continue;
			if (local) {
				atomicAdd(lb + kTallyLds + id, 1u);
				if (j == 0)
					atomicAdd(lb + id, 1u);
			} else {
				atomicAdd(any + id, 1ull);
				if (j == 0)
					atomicAdd(best + id, 1ull);
			}
		}
	}
	rows = wave_sum(rows);
	none = wave_sum(none);
	multi = wave_sum(multi);
	trunc = wave_sum(trunc);
	sat = wave_sum64(sat);
	ev = wave_sum64(ev);
	if ((threadIdx.x & 63) == 0 && rows) {
		atomicAdd(totals + 0, (unsigned long long)rows);
		if (none)
			atomicAdd(totals + 1, (unsigned long long)none);
		if (multi)
			atomicAdd(totals + 2, (unsigned long long)multi);
		if (trunc)
			atomicAdd(totals + 3, (unsigned long long)trunc);
		if (sat)
			atomicAdd(totals + 4, sat);
		if (ev)
			atomicAdd(totals + 5, ev);
	}
	__syncthreads();
	if (local)
		for (uint32_t b = threadIdx.x; b < (uint32_t)n_ids; b += blockDim.x) {
			if (lb[b])
				atomicAdd(best + b, (unsigned long long)lb[b]);
			if (lb[kTallyLds + b])
				atomicAdd(any + b, (unsigned long long)lb[kTallyLds + b]);
		}
}

hipError_t launch_mibf_tally(const void* hits, const uint32_t* n_hits, const uint32_t* sat_count,
                             const uint32_t* eval_count, uint64_t n_rows, uint32_t max_results, uint64_t n_ids,
                             unsigned long long* best, unsigned long long* any, unsigned long long* totals, hipStream_t s)
{
	if (n_rows == 0)
		return hipSuccess;
	// few workgroups when they carry LDS bins to flush: n_ids atomics each
	const uint64_t blocks = std::min<uint64_t>((n_rows + 255) / 256, 512);
	hipLaunchKernelGGL(mibf_tally_kernel, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint32_t*>(hits),
	                   n_hits, sat_count, eval_count, n_rows, max_results, n_ids, best, any, totals);
	return hipGetLastError();
}

} // namespace btlbf
