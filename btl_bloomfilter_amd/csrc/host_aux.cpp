// csrc/host_aux.cpp -- what surrounds the filters: popcount / digest / compare, the rank structure, the position
// exchange helpers of the sharded filter, synthetic reads and the micro-benchmarks (kernels: aux_kernels.hip).
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace btlbf;

// -------------------------------------------------------------------------------------------------
// statistics
// -------------------------------------------------------------------------------------------------
static int popcount_mode(btlbf_filter* f, int mode, uint64_t* out)
{
	if (!f || !out)
		return fail(BTLBF_EINVAL, "null argument");
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize()); // DEVICE-mode calls may have run on non-blocking user streams
	HIP_TRY(hipMemset(f->d_scalar, 0, 8));
	const unsigned cb = is_wide(f) ? counter_bytes(f) : 1;
	if (cb > 1)
		HIP_TRY(launch_wide_popcount(f->d_data, f->alloc_bytes, (int)cb, mode, f->thr, f->d_scalar, nullptr));
	else
		HIP_TRY(launch_popcount(f->d_data, f->alloc_bytes, mode, f->thr, f->d_scalar, nullptr));
	unsigned long long v = 0;
	HIP_TRY(hipMemcpy(&v, f->d_scalar, 8, hipMemcpyDeviceToHost));
	if (mode == 2 && f->thr == 0)
		v -= (f->alloc_bytes - f->local_bytes) / cb; // zero padding also passes ">= 0"
	*out = v;
	return BTLBF_OK;
}

extern "C" int btlbf_popcount(btlbf_filter* f, uint64_t* out)
{
	FilterLock lk__(f);
	return popcount_mode(f, f && is_counting(f) ? 1 : 0, out);
}

extern "C" int btlbf_filtered_popcount(btlbf_filter* f, uint64_t* out)
{
	FilterLock lk__(f);
	if (f && !is_counting(f))
		return fail(BTLBF_EINVAL, "filtered_popcount needs a counting filter");
	return popcount_mode(f, 2, out);
}

extern "C" int btlbf_digest(btlbf_filter* f, uint64_t* out2)
{
	FilterLock lk__(f);
	if (!f || !out2)
		return fail(BTLBF_EINVAL, "null argument");
	// the first local position must start a 64-bit word of the whole array (shards are cut at multiples of 64)
	const uint64_t per_word = is_counting(f) ? 8 / counter_bytes(f) : 64;
	if (f->mod.shard_lo % per_word)
		return fail(BTLBF_EINVAL, "digest: the shard does not start on a 64-bit word of the filter");
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize()); // DEVICE-mode calls may have run on non-blocking user streams
	HIP_TRY(hipMemset(f->d_scalar, 0, 16));
	HIP_TRY(launch_digest(f->d_data, f->alloc_bytes, f->mod.shard_lo / per_word, f->d_scalar, nullptr));
	HIP_TRY(hipMemcpy(out2, f->d_scalar, 16, hipMemcpyDeviceToHost));
	return BTLBF_OK;
}

extern "C" int btlbf_compare(btlbf_filter* a, btlbf_filter* b, uint64_t* out3)
{
	if (!a || !b || !out3)
		return fail(BTLBF_EINVAL, "null argument");
	FilterLock lk1__(a < b ? a : b), lk2__(a == b ? nullptr : (a < b ? b : a));
	if (a->kind != b->kind || a->size != b->size || a->local_bytes != b->local_bytes ||
	    a->mod.shard_lo != b->mod.shard_lo || a->device != b->device)
		return fail(BTLBF_EINVAL, "btlbf_compare: the two filters differ in kind, size, shard range or device");
	DeviceGuard g(a->device);
	MATERIALIZE(a, nullptr);
	MATERIALIZE(b, nullptr);
	HIP_TRY(hipDeviceSynchronize()); // whatever streams the two filters were last used on
	DevBuf acc;
	HIP_TRY(acc.alloc(24));
	HIP_TRY(hipMemset(acc.p, 0, 24));
	if (is_wide(a))
		HIP_TRY(launch_wide_compare(a->d_data, b->d_data, a->alloc_bytes, (int)counter_bytes(a),
		                            acc.as<unsigned long long>(), nullptr));
	else
		HIP_TRY(launch_compare(a->d_data, b->d_data, a->alloc_bytes, a->kind == BTLBF_COUNTING8,
		                       acc.as<unsigned long long>(), nullptr));
	unsigned long long v[3] = {0, 0, 0};
	HIP_TRY(hipMemcpy(v, acc.p, 24, hipMemcpyDeviceToHost));
	out3[0] = v[0];
	out3[1] = v[1];
	out3[2] = v[2];
	return BTLBF_OK;
}

// -------------------------------------------------------------------------------------------------
// rank structure (miBF stage 2)
// -------------------------------------------------------------------------------------------------
struct btlbf_rank {
	int device = 0;
	uint64_t n_bits = 0, n_blocks = 0, ones = 0;
	ModParams mod{};
	uint64_t* d_il = nullptr; // n_blocks records of 9 uint64_t
};

namespace btlbf {
// the one build of the rank structure, for btlbf_rank_create and the miBF (host_internal.hpp has the contract)
hipError_t rank_build(const btlbf_filter* f, uint64_t** d_il, uint64_t* n_blocks, uint64_t* ones)
{
	*n_blocks = (f->size + 511) / 512;
	*d_il = nullptr;
	DevBuf scratch;
	hipError_t e = hipMalloc((void**)d_il, *n_blocks * 9 * 8 + 16);
	if (e == hipSuccess && (e = scratch.alloc((*n_blocks + (*n_blocks + 4095) / 4096 + 2) * 8)) != hipSuccess) {
		(void)hipFree(*d_il);
		*d_il = nullptr;
	}
	if (e != hipSuccess)
		return e;
	uint64_t* total = scratch.as<uint64_t>() + *n_blocks + (*n_blocks + 4095) / 4096;
	e = launch_rank_build(static_cast<const uint64_t*>(f->d_data), f->size, *d_il, scratch.as<uint64_t>(), total, nullptr);
	if (e == hipSuccess)
		e = hipMemcpy(ones, total, 8, hipMemcpyDeviceToHost);
	return e;
}
} // namespace btlbf

extern "C" int btlbf_rank_create(btlbf_rank** out, btlbf_filter* f)
{
	if (!out || !f)
		return fail(BTLBF_EINVAL, "null argument");
	*out = nullptr;
	if (f->kind != BTLBF_BLOOM || f->shard_count != 1)
		return fail(BTLBF_EINVAL, "rank structure: needs a whole bit filter");
	FilterLock lk__(f);
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize());
	btlbf_rank* r = new btlbf_rank();
	r->device = f->device;
	r->n_bits = f->size;
	fill_mod(r->mod, f->size, 0, f->size);
	hipError_t e = rank_build(f, &r->d_il, &r->n_blocks, &r->ones);
	if (e != hipSuccess && !r->d_il) {
		const unsigned long long bytes = r->n_blocks * 72;
		delete r;
		(void)hipGetLastError();
		return fail(BTLBF_ENOMEM, "rank structure: %llu bytes of HBM", bytes);
	}
	if (e != hipSuccess) {
		(void)hipFree(r->d_il);
		delete r;
		return fail(BTLBF_EHIP, "rank structure: %s", hipGetErrorString(e));
	}
	*out = r;
	return BTLBF_OK;
}

extern "C" void btlbf_rank_destroy(btlbf_rank* r)
{
	if (!r)
		return;
	DeviceGuard g(r->device);
	(void)hipFree(r->d_il);
	delete r;
}

extern "C" uint64_t btlbf_rank_ones(const btlbf_rank* r) { return r ? r->ones : 0; }
extern "C" uint64_t btlbf_rank_words(const btlbf_rank* r) { return r ? r->n_blocks * 9 : 0; }

extern "C" int btlbf_rank_download(const btlbf_rank* r, uint64_t* host_dst)
{
	if (!r || !host_dst)
		return fail(BTLBF_EINVAL, "null argument");
	DeviceGuard g(r->device);
	HIP_TRY(hipMemcpy(host_dst, r->d_il, r->n_blocks * 72, hipMemcpyDeviceToHost));
	return BTLBF_OK;
}

extern "C" int btlbf_rank_query(const btlbf_rank* r, const uint64_t* values, uint64_t n, int values_are_hashes,
                                uint64_t* rank_out, uint8_t* bit_out, int mem, void* stream)
{
	if (!r || (n && !values))
		return fail(BTLBF_EINVAL, "null argument");
	if (mem != BTLBF_HOST && mem != BTLBF_DEVICE)
		return fail(BTLBF_EINVAL, "mem must be BTLBF_HOST or BTLBF_DEVICE");
	DeviceGuard g(r->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	DevBuf din;
	const uint64_t* dv = values;
	if (mem == BTLBF_HOST) {
		HIP_TRY(din.alloc(n * 8));
		if (n)
			HIP_TRY(hipMemcpyAsync(din.p, values, n * 8, hipMemcpyHostToDevice, s));
		dv = din.as<uint64_t>();
	}
	OutBuf o_rank, o_bit;
	int rc;
	if ((rc = o_rank.prepare(rank_out, n * 8, mem, false, s)) || (rc = o_bit.prepare(bit_out, n, mem, false, s)))
		return rc;
	HIP_TRY(launch_rank_query(r->d_il, r->n_bits, dv, n, r->mod, values_are_hashes, static_cast<uint64_t*>(o_rank.d),
	                          static_cast<uint8_t*>(o_bit.d), s));
	if ((rc = o_rank.finish(s)) || (rc = o_bit.finish(s)))
		return rc;
	if (mem == BTLBF_HOST)
		HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

// -------------------------------------------------------------------------------------------------
// multi-GPU helpers
// -------------------------------------------------------------------------------------------------
extern "C" int btlbf_positions_seqs(btlbf_filter* f, const char* seq, uint64_t len,
                                    const btlbf_layout* layout, unsigned n_shards, uint64_t* buckets,
                                    uint64_t* tags, uint64_t bucket_cap, uint64_t* bucket_counts,
                                    uint64_t* valid_bits, void* stream)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_positions_seqs");
	int rc = seq_precheck(f);
	if (rc)
		return rc;
	if (!buckets || !bucket_counts || n_shards == 0 || n_shards > 64)
		return fail(BTLBF_EINVAL, "bad bucket arguments");
	if (f->size % n_shards)
		return fail(BTLBF_EINVAL, "size not divisible by n_shards");
	DeviceGuard g(f->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	SeqView v;
	rc = make_view(v, seq, len, layout, BTLBF_DEVICE, s);
	if (rc)
		return rc;
	SeqArgs a = base_args(f, v, len);
	fill_mod(a.mod, f->size, 0, f->size / n_shards); // owner = position / (size/n_shards)
	a.n_shards = n_shards;
	a.buckets = buckets;
	a.tags = tags;
	a.bucket_cap = bucket_cap;
	a.bucket_counts = reinterpret_cast<unsigned long long*>(bucket_counts);
	a.valid_bits = reinterpret_cast<uint8_t*>(valid_bits);
	HIP_TRY(hipMemsetAsync(bucket_counts, 0, (size_t)n_shards * 8, s));
	HIP_TRY(launch_seq_op(OP_POSITIONS, a, s));
	return BTLBF_OK;
}

extern "C" int btlbf_insert_positions(btlbf_filter* f, const uint64_t* local_pos, uint64_t n, void* stream)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_insert_positions");
	if (!f || (n && !local_pos))
		return fail(BTLBF_EINVAL, "null argument");
	if (f->kind != BTLBF_BLOOM)
		return fail(BTLBF_EINVAL, "position routing is defined for bit filters");
	DeviceGuard g(f->device);
	MATERIALIZE(f, stream);
	HIP_TRY(launch_positions(0, f->d_data, f->mod, local_pos, n, nullptr, static_cast<hipStream_t>(stream)));
	return BTLBF_OK;
}

extern "C" int btlbf_test_positions(btlbf_filter* f, const uint64_t* local_pos, uint64_t n, uint8_t* out,
                                    void* stream)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_test_positions");
	if (!f || (n && (!local_pos || !out)))
		return fail(BTLBF_EINVAL, "null argument");
	if (f->kind != BTLBF_BLOOM)
		return fail(BTLBF_EINVAL, "position routing is defined for bit filters");
	DeviceGuard g(f->device);
	MATERIALIZE(f, stream);
	HIP_TRY(launch_positions(1, f->d_data, f->mod, local_pos, n, out, static_cast<hipStream_t>(stream)));
	return BTLBF_OK;
}

extern "C" int btlbf_and_answers(const uint64_t* tags, const uint8_t* answers, uint64_t n, unsigned hash_num,
                                 uint64_t* hit_bits, int device, void* stream)
{
	if (n && (!tags || !answers || !hit_bits))
		return fail(BTLBF_EINVAL, "null argument");
	DeviceGuard g(device);
	HIP_TRY(launch_and_answers(tags, answers, n, hash_num, hit_bits, static_cast<hipStream_t>(stream)));
	return BTLBF_OK;
}

extern "C" int btlbf_count_per_seq(const uint64_t* hit_bits, const uint64_t* valid_bits, uint64_t len,
                                   const btlbf_layout* layout, unsigned kmer_size, uint32_t* hits_out,
                                   uint32_t* valid_out, int mem, int device, void* stream)
{
	if (!layout || (!layout->starts && !layout->read_len))
		return fail(BTLBF_EINVAL, "count_per_seq needs a layout (starts[] or read_len)");
	if (kmer_size == 0 || (len && (!hit_bits || !hits_out)))
		return fail(BTLBF_EINVAL, "null argument");
	int rc = check_layout(layout, len);
	if (rc)
		return rc;
	const uint64_t n_seqs = layout->starts ? layout->n_seqs : len / layout->read_len;
	if (n_seqs == 0)
		return BTLBF_OK;
	if (mem != BTLBF_HOST && mem != BTLBF_DEVICE)
		return fail(BTLBF_EINVAL, "mem must be BTLBF_HOST or BTLBF_DEVICE");
	DeviceGuard g(device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	const size_t bm = bitmap_bytes(len);
	DevBuf d_hit, d_valid, d_starts, d_ho, d_vo;
	const uint64_t *ph = hit_bits, *pv = valid_bits, *ps = layout->starts;
	uint32_t *po = hits_out, *pvo = valid_out;
	if (mem == BTLBF_HOST) {
		HIP_TRY(d_hit.alloc(bm));
		HIP_TRY(hipMemcpyAsync(d_hit.p, hit_bits, bm, hipMemcpyHostToDevice, s));
		ph = d_hit.as<uint64_t>();
		if (valid_bits) {
			HIP_TRY(d_valid.alloc(bm));
			HIP_TRY(hipMemcpyAsync(d_valid.p, valid_bits, bm, hipMemcpyHostToDevice, s));
			pv = d_valid.as<uint64_t>();
		}
		if (layout->starts) {
			HIP_TRY(d_starts.alloc((n_seqs + 1) * 8));
			HIP_TRY(hipMemcpyAsync(d_starts.p, layout->starts, (n_seqs + 1) * 8, hipMemcpyHostToDevice, s));
			ps = d_starts.as<uint64_t>();
		}
		HIP_TRY(d_ho.alloc(n_seqs * 4));
		po = d_ho.as<uint32_t>();
		if (valid_out) {
			HIP_TRY(d_vo.alloc(n_seqs * 4));
			pvo = d_vo.as<uint32_t>();
		}
	}
	HIP_TRY(launch_count_per_seq(ph, pv, len, ps, n_seqs, layout->starts ? 0 : layout->read_len, kmer_size, po, pvo, s));
	if (mem == BTLBF_HOST) {
		HIP_TRY(hipMemcpyAsync(hits_out, po, n_seqs * 4, hipMemcpyDeviceToHost, s));
		if (valid_out)
			HIP_TRY(hipMemcpyAsync(valid_out, pvo, n_seqs * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
	}
	return BTLBF_OK;
}

extern "C" int btlbf_popcount_bits(const void* dev_buf, uint64_t nbytes, uint64_t* out, int device,
                                   void* stream)
{
	if (!out || (nbytes && !dev_buf))
		return fail(BTLBF_EINVAL, "null argument");
	if (nbytes % 8)
		return fail(BTLBF_EINVAL, "nbytes must be a multiple of 8");
	DeviceGuard g(device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	DevBuf acc;
	HIP_TRY(acc.alloc(8));
	HIP_TRY(hipMemsetAsync(acc.p, 0, 8, s));
	HIP_TRY(launch_popcount(dev_buf, nbytes, 0, 0, acc.as<unsigned long long>(), s));
	unsigned long long v = 0;
	HIP_TRY(hipMemcpyAsync(&v, acc.p, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	*out = v;
	return BTLBF_OK;
}

// -------------------------------------------------------------------------------------------------
// support
// -------------------------------------------------------------------------------------------------
extern "C" int btlbf_synth_reads(char* dev_out, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                                 unsigned read_len, int device, void* stream)
{
	if (!dev_out || read_len == 0)
		return fail(BTLBF_EINVAL, "bad argument");
	DeviceGuard g(device);
	HIP_TRY(launch_synth(reinterpret_cast<uint8_t*>(dev_out), seed, first_read, n_reads, read_len,
	                     static_cast<hipStream_t>(stream)));
	return BTLBF_OK;
}

extern "C" int btlbf_microbench(btlbf_filter* f, int kind, uint64_t n_access, uint64_t* n_done,
                                double* seconds)
{
	FilterLock lk__(f);
	if (f && is_wide(f))
		return refuse_wide("btlbf_microbench");
	if (!f || !seconds || !n_done)
		return fail(BTLBF_EINVAL, "null argument");
	{
		const uint64_t per_round = 2048ull * 256 * 8; // launch_microbench geometry
		uint64_t rounds = n_access / per_round;
		*n_done = (rounds ? rounds : 1) * per_round;
	}
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize()); // DEVICE-mode calls may have run on non-blocking user streams
	hipEvent_t e0, e1;
	HIP_TRY(hipEventCreate(&e0));
	HIP_TRY(hipEventCreate(&e1));
	HIP_TRY(hipMemset(f->d_scalar, 0, 8));
	HIP_TRY(hipEventRecord(e0, nullptr));
	HIP_TRY(launch_microbench(f->d_data, f->local_bytes, kind, n_access, f->d_scalar, nullptr));
	HIP_TRY(hipEventRecord(e1, nullptr));
	HIP_TRY(hipEventSynchronize(e1));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
	(void)hipEventDestroy(e0);
	(void)hipEventDestroy(e1);
	*seconds = ms * 1e-3;
	return BTLBF_OK;
}
