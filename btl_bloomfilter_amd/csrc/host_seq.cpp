// csrc/host_seq.cpp -- the compute entry points over sequences, precomputed hash rows and raw k-mers.
//
// run_query_like is the hot path of every query flavour: the mailbox fast path for a short host sequence, else staged
// buffers and, for contains(), the routed query (host_query.cpp's contains_routed, which picks between the direct
// kernels, the partitioned pipeline and the split routes); what it leaves unanswered, and every other flavour, is the one
// whole-buffer launch of the direct kernel here.  Inserts enter the partitioned pipeline (host_partition.cpp) through
// want_partitioned and partitioned_insert.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"

#include <cstring>
#include <vector>

using namespace btlbf;

// -------------------------------------------------------------------------------------------------
// the hot path
// -------------------------------------------------------------------------------------------------
namespace btlbf {

int seq_precheck(const btlbf_filter* f)
{
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	if (f->hp.n_seeds == 0 && f->h > 64)
		return fail(BTLBF_EINVAL, "hash_num %u > 64 unsupported by the sequence kernels", f->h);
	return BTLBF_OK;
}

} // namespace btlbf

namespace {

// the one whole-buffer launch of a query flavour: the fused kernel of the filter's counter width
hipError_t launch_query(const btlbf_filter* f, int op, const SeqArgs& a, hipStream_t s)
{
	return is_wide(f) ? launch_wide_seq_op(W_QUERY, (int)counter_bytes(f), a, s) : launch_seq_op(op, a, s);
}

// min_out: len elements of min_width bytes each (the filter's counter width; 1 for the byte forms)
int run_query_like(btlbf_filter* f, int op, const char* seq, uint64_t len, const btlbf_layout* layout,
                   uint64_t* hit_bits, uint64_t* valid_bits, uint64_t* counts, void* min_out, int mem,
                   void* stream, FilterLock* lk = nullptr, unsigned min_width = 1)
{
	int rc = seq_precheck(f);
	if (rc)
		return rc;
	// contains() on a shard answers for the probes inside its window (ShardedBloomFilter's gather mode
	// ANDs the shards' answers); the other query flavours need all h probes of a k-mer
	if (f->shard_count != 1) {
		if (op != OP_BF_CONTAINS && !(op == OP_CBF_QUERY && !min_out))
			return fail(BTLBF_EINVAL, "this query on a shard goes through btlbf_positions_seqs/btlbf_test_positions");
		if (op == OP_BF_CONTAINS)
			op = OP_BF_CONTAINS_WIN;
	}
	DeviceGuard g(f->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	MATERIALIZE(f, s);
	// a short sequence from host memory (the shims' per-read containsSeq / countSeq): through the calling thread's
	// pinned mailbox with the direct kernel -- one launch, one synchronisation, no staging (such a batch is far
	// below what the partitioned path takes)
	{
		const uint64_t up16 = ~(uint64_t)15, bm = (bitmap_bytes(len) + 15) & up16;
		const uint64_t o_hit = (len + 16 + 15) & up16, o_valid = o_hit + bm, o_cnt = o_valid + bm, o_min = o_cnt + 16,
		               o_end = o_min + ((len * min_width + 15) & up16);
		if (mem == BTLBF_HOST && len && len <= 65536 && (!layout || !layout->starts) && o_end <= Mailbox::kBytes &&
		    mailbox().get()) {
			if ((rc = check_layout(layout, len)))
				return rc;
			Mailbox& mb = mailbox();
			memcpy(mb.host, seq, len);
			SeqView v;
			v.d_seq = mb.dev;
			v.lay.read_len = layout ? layout->read_len : 0;
			SeqArgs a = base_args(f, v, len);
			// {clean windows, hits} are counted on the host from the two bitmaps (no atomics into host memory)
			a.hit_bits = hit_bits || counts ? mb.dev + o_hit : nullptr;
			a.valid_bits = valid_bits || counts ? mb.dev + o_valid : nullptr;
			a.min_out = min_out ? mb.dev + o_min : nullptr;
			REQUIRE_MATERIALIZED(f);
			HIP_TRY(launch_query(f, op, a, s));
			if (lk && op != OP_BF_INSERT_CHECK)
				lk->release(); // a read-only call only waits from here on (its mailbox is the calling thread's own)
			HIP_TRY(hipStreamSynchronize(s));
			if (hit_bits)
				memcpy(hit_bits, mb.host + o_hit, bitmap_bytes(len));
			if (valid_bits)
				memcpy(valid_bits, mb.host + o_valid, bitmap_bytes(len));
			if (counts) {
				counts[0] = counts[1] = 0;
				const uint64_t* hb = reinterpret_cast<const uint64_t*>(mb.host + o_hit);
				const uint64_t* vb = reinterpret_cast<const uint64_t*>(mb.host + o_valid);
				for (uint64_t i = 0; i < bitmap_bytes(len) / 8; ++i) {
					counts[0] += (uint64_t)__builtin_popcountll(vb[i]);
					counts[1] += (uint64_t)__builtin_popcountll(hb[i]);
				}
			}
			if (min_out)
				memcpy(min_out, mb.host + o_min, len * min_width);
			return BTLBF_OK;
		}
	}
	SeqView v;
	rc = make_view(v, seq, len, layout, mem, s);
	if (rc)
		return rc;
	OutBuf ob_hit, ob_valid, ob_cnt, ob_min;
	if ((rc = ob_hit.prepare(hit_bits, bitmap_bytes(len), mem, false, s)))
		return rc;
	if ((rc = ob_valid.prepare(valid_bits, bitmap_bytes(len), mem, false, s)))
		return rc;
	if ((rc = ob_cnt.prepare(counts, 16, mem, true, s)))
		return rc;
	if ((rc = ob_min.prepare(min_out, len * min_width, mem, false, s)))
		return rc;
	SeqArgs a = base_args(f, v, len);
	a.hit_bits = static_cast<uint8_t*>(ob_hit.d);
	a.valid_bits = static_cast<uint8_t*>(ob_valid.d);
	a.counts = static_cast<uint64_t*>(ob_cnt.d);
	a.min_out = static_cast<uint8_t*>(ob_min.d);
	bool answered = false;
	// minimum counts need the values, and wide counters have the direct path only: neither is routed
	if (!is_wide(f) && (op == OP_BF_CONTAINS || op == OP_BF_CONTAINS_WIN || (op == OP_CBF_QUERY && !min_out))) {
		if ((rc = contains_routed(f, a, op, s, &answered)))
			return rc;
	}
	if (!answered) {
		REQUIRE_MATERIALIZED(f);
		ProfSpan ps(f, op == OP_BF_CONTAINS || op == OP_BF_CONTAINS_WIN ? BTLBF_PROF_QUERY_DIRECT : BTLBF_PROF_OTHER, s);
		HIP_TRY(launch_query(f, op, a, s));
	}
	if ((rc = ob_hit.finish(s)) || (rc = ob_valid.finish(s)) || (rc = ob_cnt.finish(s)) ||
	    (rc = ob_min.finish(s)))
		return rc;
	if (mem == BTLBF_HOST)
		HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

// the launch of a hash-row operation on the filter's counter width (row_valid: raw k-mers without a defined value)
hipError_t launch_rows(const btlbf_filter* f, int hop, const uint64_t* rows, uint64_t n, void* out, int serial,
                       hipStream_t s, const uint8_t* row_valid = nullptr)
{
	if (is_wide(f))
		return launch_wide_hash_op(hop, (int)counter_bytes(f), f->d_data, f->mod, f->h, f->thr, rows, n, out, serial, s,
		                           row_valid);
	return launch_hash_op(hop, f->d_data, f->mod, f->h, f->thr, rows, n, static_cast<uint8_t*>(out), serial, s, row_valid);
}

// out: n elements of out_width bytes each (1, or the counter width for the minimum counts of a wide filter)
int run_hash_rows(btlbf_filter* f, int hop, const uint64_t* hashes, uint64_t n, void* out, int serial,
                  int mem, void* stream, FilterLock* lk = nullptr, unsigned out_width = 1)
{
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	if (n && !hashes)
		return fail(BTLBF_EINVAL, "null hashes");
	if (f->shard_count != 1 && hop != H_BF_INSERT)
		return fail(BTLBF_EINVAL, "only insert is defined on a single shard");
	DeviceGuard g(f->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	MATERIALIZE(f, s);
	// a few rows from host memory (the shims' per-k-mer contains / insertAndCheck / minCount): through the calling
	// thread's pinned mailbox -- no staging buffers, no copies, one launch and one synchronisation
	const uint64_t row_bytes = (n * f->h * 8 + 15) & ~(uint64_t)15;
	if (mem == BTLBF_HOST && n && row_bytes + n * out_width <= Mailbox::kBytes && mailbox().get()) {
		Mailbox& mb = mailbox();
		memcpy(mb.host, hashes, n * f->h * 8);
		REQUIRE_MATERIALIZED(f);
		HIP_TRY(launch_rows(f, hop, reinterpret_cast<const uint64_t*>(mb.dev), n, out ? mb.dev + row_bytes : nullptr, serial,
		                    s));
		if (lk && (hop == H_BF_CONTAINS || hop == H_CBF_CONTAINS || hop == H_CBF_MIN))
			lk->release(); // the mailbox and (with BTLBF_STREAM_PER_THREAD) the stream are the calling thread's own
		HIP_TRY(hipStreamSynchronize(s));
		if (out)
			memcpy(out, mb.host + row_bytes, n * out_width);
		return BTLBF_OK;
	}
	DevBuf hb;
	const uint64_t* d_h = hashes;
	if (mem == BTLBF_HOST) {
		HIP_TRY(hb.alloc_pooled(n * f->h * 8));
		if (n)
			HIP_TRY(hipMemcpyAsync(hb.p, hashes, n * f->h * 8, hipMemcpyHostToDevice, s));
		d_h = hb.as<uint64_t>();
	}
	OutBuf ob;
	int rc = ob.prepare(out, n * out_width, mem, false, s);
	if (rc)
		return rc;
	REQUIRE_MATERIALIZED(f);
	HIP_TRY(launch_rows(f, hop, d_h, n, ob.d, serial, s));
	if ((rc = ob.finish(s)))
		return rc;
	if (mem == BTLBF_HOST)
		HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

// n k-mers of k bytes each -> device hash rows + valid bytes (aux_kernels.hip, kmer_rows_kernel)
struct KmerRows {
	DevBuf seq, rows, valid;
	const uint8_t* d_seq = nullptr;
	int prepare(const char* kmers, uint64_t n, unsigned k, unsigned h, uint64_t kms, int mem, hipStream_t s)
	{
		if (n && !kmers)
			return fail(BTLBF_EINVAL, "null kmers");
		d_seq = reinterpret_cast<const uint8_t*>(kmers);
		if (mem == BTLBF_HOST) {
			HIP_TRY(seq.alloc_pooled(n * k));
			if (n)
				HIP_TRY(hipMemcpyAsync(seq.p, kmers, n * k, hipMemcpyHostToDevice, s));
			d_seq = seq.as<uint8_t>();
		}
		HIP_TRY(rows.alloc_pooled(n * h * 8));
		HIP_TRY(valid.alloc_pooled(n));
		HIP_TRY(launch_kmer_rows(d_seq, n, k, h, kms, rows.as<uint64_t>(), valid.as<uint8_t>(), s));
		return BTLBF_OK;
	}
};

int run_kmer_rows(btlbf_filter* f, int hop, const char* kmers, uint64_t n, uint8_t* out, int serial, int mem,
                  void* stream)
{
	if (f->hp.n_seeds)
		return fail(BTLBF_EINVAL, "raw k-mers are hashed with ntHash, not with spaced seeds");
	if (f->shard_count != 1 && hop != H_BF_INSERT)
		return fail(BTLBF_EINVAL, "only insert is defined on a single shard");
	DeviceGuard g(f->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	MATERIALIZE(f, s);
	KmerRows kr;
	int rc = kr.prepare(kmers, n, f->k, f->h, f->hp.kms, mem, s);
	if (rc)
		return rc;
	OutBuf ob;
	if ((rc = ob.prepare(out, n, mem, false, s)))
		return rc;
	HIP_TRY(launch_rows(f, hop, kr.rows.as<uint64_t>(), n, ob.d, serial, s, kr.valid.as<uint8_t>()));
	if ((rc = ob.finish(s)))
		return rc;
	HIP_TRY(hipStreamSynchronize(s)); // the temporaries are freed on return
	return BTLBF_OK;
}

// try the partitioned insert of `a`; *done: it ran, and a call from host memory has waited for it (false: the scratch does
// not fit, nothing was launched, the caller goes on to the direct kernels)
int try_partitioned_insert(btlbf_filter* f, const SeqArgs& a, int mem, hipStream_t s, bool* done)
{
	if (int rc = partitioned_insert(f, a, s, done))
		return rc;
	if (*done && mem == BTLBF_HOST)
		HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

} // namespace

extern "C" int btlbf_insert_seqs(btlbf_filter* f, const char* seq, uint64_t len,
                                 const btlbf_layout* layout, int op, int order, int mem, void* stream)
{
	FilterLock lk__(f);
	int rc = seq_precheck(f);
	if (rc)
		return rc;
	DeviceGuard g(f->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	SeqView v;
	rc = make_view(v, seq, len, layout, mem, s);
	if (rc)
		return rc;
	SeqArgs a = base_args(f, v, len);
	int kop;
	if (f->kind == BTLBF_BLOOM) {
		kop = OP_BF_INSERT; // bit OR is order-free: serial order would give the same bytes
		if (want_partitioned(f, len)) {
			bool done = false;
			if ((rc = try_partitioned_insert(f, a, mem, s, &done)) || done)
				return rc;
		}
		MATERIALIZE(f, s);
	} else {
		// a counting shard keeps the increments inside its window; the conservative update needs all h
		// counters of a k-mer, which live on different shards
		if (f->shard_count != 1 && (op != BTLBF_INCREMENT_ALL || order == BTLBF_ORDER_SERIAL))
			return fail(BTLBF_EINVAL, "a counting-filter shard takes incrementAll in parallel order only");
		if (op != BTLBF_INCREMENT_MIN && op != BTLBF_INCREMENT_ALL)
			return fail(BTLBF_EINVAL, "op must be BTLBF_INCREMENT_MIN or BTLBF_INCREMENT_ALL");
		kop = op == BTLBF_INCREMENT_MIN ? OP_CBF_INC_MIN : OP_CBF_INC_ALL;
		if (order != BTLBF_ORDER_SERIAL && want_partitioned(f, len, op)) {
			// incrementAll is order-free up to saturation, which is order-free too: exact in any order
			bool done = false;
			if ((rc = try_partitioned_insert(f, a, mem, s, &done)) || done)
				return rc;
		}
		MATERIALIZE(f, s);
		if (order == BTLBF_ORDER_SERIAL) {
			// hash on all CUs, then apply the rows in buffer order on a single lane
			DevBuf hashes, valid;
			HIP_TRY(hashes.alloc(len * f->h * 8));
			HIP_TRY(valid.alloc(bitmap_bytes(len)));
			a.hashes = hashes.as<uint64_t>();
			a.valid_bits = valid.as<uint8_t>();
			HIP_TRY(launch_seq_op(OP_HASH_ONLY, a, s));
			const int hop = op == BTLBF_INCREMENT_MIN ? H_CBF_INC_MIN : H_CBF_INC_ALL;
			if (is_wide(f))
				HIP_TRY(launch_wide_serial_seq_update((int)counter_bytes(f), a, hop, hashes.as<uint64_t>(),
				                                      valid.as<uint8_t>(), s));
			else
				HIP_TRY(launch_serial_seq_update(a, hop, hashes.as<uint64_t>(), valid.as<uint8_t>(), nullptr, s));
			HIP_TRY(hipStreamSynchronize(s));
			return BTLBF_OK;
		}
	}
	{
		REQUIRE_MATERIALIZED(f);
		ProfSpan ps(f, kop == OP_BF_INSERT ? BTLBF_PROF_INSERT_DIRECT : BTLBF_PROF_OTHER, s);
		if (is_wide(f))
			HIP_TRY(launch_wide_seq_op(kop == OP_CBF_INC_MIN ? W_INC_MIN : W_INC_ALL, (int)counter_bytes(f), a, s));
		else
			HIP_TRY(launch_seq_op(kop, a, s));
	}
	if (mem == BTLBF_HOST)
		HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

extern "C" int btlbf_contains_seqs(btlbf_filter* f, const char* seq, uint64_t len,
                                   const btlbf_layout* layout, uint64_t* hit_bits, uint64_t* valid_bits,
                                   uint64_t* counts, int mem, void* stream)
{
	FilterLock lk__(f);
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	return run_query_like(f, f->kind == BTLBF_BLOOM ? OP_BF_CONTAINS : OP_CBF_QUERY, seq, len, layout,
	                      hit_bits, valid_bits, counts, nullptr, mem, stream, &lk__);
}

extern "C" int btlbf_insert_and_check_seqs(btlbf_filter* f, const char* seq, uint64_t len,
                                           const btlbf_layout* layout, uint64_t* hit_bits,
                                           uint64_t* valid_bits, uint64_t* counts, int mem, void* stream)
{
	FilterLock lk__(f);
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	if (f->kind != BTLBF_BLOOM)
		return fail(BTLBF_EINVAL, "insert_and_check_seqs: bit filters only (use the hash-row form for counting)");
	return run_query_like(f, OP_BF_INSERT_CHECK, seq, len, layout, hit_bits, valid_bits, counts, nullptr, mem,
	                      stream);
}

extern "C" int btlbf_min_count_seqs(btlbf_filter* f, const char* seq, uint64_t len,
                                    const btlbf_layout* layout, uint8_t* min_out, uint64_t* valid_bits,
                                    int mem, void* stream)
{
	FilterLock lk__(f);
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	if (is_wide(f)) // before any HIP call, nothing written: the caller's bytes would be overrun
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_min_count_seqs: the filter's counters have %u bytes, use "
		                                     "btlbf_min_count_seqs_wide", counter_bytes(f));
	if (f->kind != BTLBF_COUNTING8)
		return fail(BTLBF_EINVAL, "min_count needs a counting filter");
	return run_query_like(f, OP_CBF_QUERY, seq, len, layout, nullptr, valid_bits, nullptr, min_out, mem, stream);
}

extern "C" int btlbf_min_count_seqs_wide(btlbf_filter* f, const char* seq, uint64_t len, const btlbf_layout* layout,
                                         void* min_out, uint64_t* valid_bits, int mem, void* stream)
{
	FilterLock lk__(f);
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	if (!is_counting(f))
		return fail(BTLBF_EINVAL, "min_count needs a counting filter");
	return run_query_like(f, OP_CBF_QUERY, seq, len, layout, nullptr, valid_bits, nullptr, min_out, mem, stream, nullptr,
	                      counter_bytes(f));
}

// -------------------------------------------------------------------------------------------------
// precomputed hash rows
// -------------------------------------------------------------------------------------------------
extern "C" int btlbf_insert_hashes(btlbf_filter* f, const uint64_t* hashes, uint64_t n, int op, int order,
                                   int mem, void* stream)
{
	FilterLock lk__(f);
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	int hop = H_BF_INSERT;
	if (is_counting(f)) {
		if (op != BTLBF_INCREMENT_MIN && op != BTLBF_INCREMENT_ALL)
			return fail(BTLBF_EINVAL, "op must be BTLBF_INCREMENT_MIN or BTLBF_INCREMENT_ALL");
		hop = op == BTLBF_INCREMENT_MIN ? H_CBF_INC_MIN : H_CBF_INC_ALL;
	}
	const int serial = is_counting(f) && order == BTLBF_ORDER_SERIAL;
	return run_hash_rows(f, hop, hashes, n, nullptr, serial, mem, stream);
}

extern "C" int btlbf_contains_hashes(btlbf_filter* f, const uint64_t* hashes, uint64_t n, uint8_t* out,
                                     int mem, void* stream)
{
	FilterLock lk__(f);
	if (!f || !out)
		return fail(BTLBF_EINVAL, "null argument");
	return run_hash_rows(f, f->kind == BTLBF_BLOOM ? H_BF_CONTAINS : H_CBF_CONTAINS, hashes, n, out, 0, mem,
	                     stream, &lk__);
}

extern "C" int btlbf_insert_and_check_hashes(btlbf_filter* f, const uint64_t* hashes, uint64_t n,
                                             uint8_t* out, int order, int mem, void* stream)
{
	FilterLock lk__(f);
	if (!f || !out)
		return fail(BTLBF_EINVAL, "null argument");
	return run_hash_rows(f, f->kind == BTLBF_BLOOM ? H_BF_INSERT_CHECK : H_CBF_INSERT_CHECK, hashes, n, out,
	                     order == BTLBF_ORDER_SERIAL, mem, stream);
}

extern "C" int btlbf_min_count_hashes(btlbf_filter* f, const uint64_t* hashes, uint64_t n, uint8_t* min_out,
                                      int mem, void* stream)
{
	FilterLock lk__(f);
	if (!f || !min_out)
		return fail(BTLBF_EINVAL, "null argument");
	if (is_wide(f)) // before any HIP call, nothing written
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_min_count_hashes: the filter's counters have %u bytes, use "
		                                     "btlbf_min_count_hashes_wide", counter_bytes(f));
	if (f->kind != BTLBF_COUNTING8)
		return fail(BTLBF_EINVAL, "min_count needs a counting filter");
	return run_hash_rows(f, H_CBF_MIN, hashes, n, min_out, 0, mem, stream);
}

extern "C" int btlbf_min_count_hashes_wide(btlbf_filter* f, const uint64_t* hashes, uint64_t n, void* min_out, int mem,
                                           void* stream)
{
	FilterLock lk__(f);
	if (!f || !min_out)
		return fail(BTLBF_EINVAL, "null argument");
	if (!is_counting(f))
		return fail(BTLBF_EINVAL, "min_count needs a counting filter");
	return run_hash_rows(f, H_CBF_MIN, hashes, n, min_out, 0, mem, stream, nullptr, counter_bytes(f));
}

// -------------------------------------------------------------------------------------------------
// raw k-mers: KmerBloomFilter::insert / contains(const char*) (KmerBloomFilter.hpp:47-74)
// -------------------------------------------------------------------------------------------------
extern "C" int btlbf_insert_kmers(btlbf_filter* f, const char* kmers, uint64_t n, int op, int order, int mem,
                                  void* stream)
{
	FilterLock lk__(f);
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	int hop = H_BF_INSERT;
	if (is_counting(f)) {
		if (op != BTLBF_INCREMENT_MIN && op != BTLBF_INCREMENT_ALL)
			return fail(BTLBF_EINVAL, "op must be BTLBF_INCREMENT_MIN or BTLBF_INCREMENT_ALL");
		hop = op == BTLBF_INCREMENT_MIN ? H_CBF_INC_MIN : H_CBF_INC_ALL;
	}
	const int serial = is_counting(f) && order == BTLBF_ORDER_SERIAL;
	return run_kmer_rows(f, hop, kmers, n, nullptr, serial, mem, stream);
}

extern "C" int btlbf_contains_kmers(btlbf_filter* f, const char* kmers, uint64_t n, uint8_t* out, int mem,
                                    void* stream)
{
	FilterLock lk__(f);
	if (!f || !out)
		return fail(BTLBF_EINVAL, "null argument");
	return run_kmer_rows(f, f->kind == BTLBF_BLOOM ? H_BF_CONTAINS : H_CBF_CONTAINS, kmers, n, out, 0, mem, stream);
}

extern "C" int btlbf_hash_kmers(unsigned kmer_size, unsigned hash_num, const char* kmers, uint64_t n,
                                uint64_t* hashes, uint8_t* valid, int mem, int device, void* stream)
{
	if (kmer_size == 0 || kmer_size > 32768 || hash_num == 0 || hash_num > 64)
		return fail(BTLBF_EINVAL, "bad kmer_size / hash_num");
	if (!hashes)
		return fail(BTLBF_EINVAL, "null hashes output");
	if (btlbf_device_count() <= device || device < 0)
		return fail(BTLBF_EHIP, "no GPU %d (visible devices: %d): this library has no CPU path", device,
		            btlbf_device_count());
	DeviceGuard g(device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	KmerRows kr;
	int rc = kr.prepare(kmers, n, kmer_size, hash_num, (uint64_t)kmer_size * kMultiSeed, mem, s);
	if (rc)
		return rc;
	const hipMemcpyKind kind = mem == BTLBF_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
	if (n) {
		HIP_TRY(hipMemcpyAsync(hashes, kr.rows.p, n * hash_num * 8, kind, s));
		if (valid)
			HIP_TRY(hipMemcpyAsync(valid, kr.valid.p, n, kind, s));
	}
	HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

// -------------------------------------------------------------------------------------------------
// hash streams only
// -------------------------------------------------------------------------------------------------
extern "C" int btlbf_hash_seqs(unsigned kmer_size, unsigned hash_num, const char* const* seeds,
                               unsigned n_seeds, unsigned h2, const char* seq, uint64_t len,
                               const btlbf_layout* layout, uint64_t* hashes, uint64_t* valid_bits,
                               uint64_t* strand_bits, int mem, int device, void* stream)
{
	if (kmer_size == 0 || kmer_size > 32768 || hash_num == 0)
		return fail(BTLBF_EINVAL, "bad kmer_size / hash_num");
	if (!seeds && hash_num > 64)
		return fail(BTLBF_EINVAL, "hash_num %u > 64 unsupported", hash_num);
	if (btlbf_device_count() <= device || device < 0)
		return fail(BTLBF_EHIP, "no GPU %d (visible devices: %d): this library has no CPU path", device,
		            btlbf_device_count());
	DeviceGuard g(device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	HashParams hp;
	fill_hash_params(hp, kmer_size, hash_num);
	DevBuf pos_owner, dc_owner;
	if (seeds) {
		if (n_seeds * h2 != hash_num)
			return fail(BTLBF_EINVAL, "hash_num must equal n_seeds*h2");
		uint64_t* dp = nullptr;
		uint16_t* dd = nullptr;
		int rc = build_spaced(hp, seeds, n_seeds, h2, &dp, &dd);
		pos_owner.p = dp;
		dc_owner.p = dd;
		if (rc)
			return rc;
	}
	if (!hashes)
		return fail(BTLBF_EINVAL, "null hashes output");
	// small host-memory calls of plain ntHash (the drop-in ntHashIterator makes one per read): through the
	// calling thread's mailbox -- the kernel reads the bases from and writes the hash rows to pinned host memory
	const uint64_t up16 = ~(uint64_t)15;
	const uint64_t o_h = (len + 16 + 15) & up16, o_v = o_h + ((len * hash_num * 8 + 15) & up16),
	               o_end = o_v + ((bitmap_bytes(len) + 15) & up16);
	if (mem == BTLBF_HOST && !seeds && !strand_bits && len && (!layout || !layout->starts) && o_end <= Mailbox::kBytes &&
	    mailbox().get()) {
		int rc = check_layout(layout, len);
		if (rc)
			return rc;
		Mailbox& mb = mailbox();
		memcpy(mb.host, seq, len);
		SeqArgs a;
		memset(&a, 0, sizeof a);
		a.seq = mb.dev;
		a.len = len;
		a.layout.read_len = layout ? layout->read_len : 0;
		a.hp = hp;
		fill_mod(a.mod, 8, 0, 8);
		a.hashes = reinterpret_cast<uint64_t*>(mb.dev + o_h);
		a.valid_bits = valid_bits ? mb.dev + o_v : nullptr;
		HIP_TRY(launch_seq_op(OP_HASH_ONLY, a, s));
		HIP_TRY(hipStreamSynchronize(s));
		memcpy(hashes, mb.host + o_h, len * hash_num * 8);
		if (valid_bits)
			memcpy(valid_bits, mb.host + o_v, bitmap_bytes(len));
		return BTLBF_OK;
	}
	SeqView v;
	int rc = make_view(v, seq, len, layout, mem, s);
	if (rc)
		return rc;
	OutBuf ob_h, ob_v, ob_s;
	if ((rc = ob_h.prepare(hashes, len * hash_num * 8, mem, false, s)))
		return rc;
	if ((rc = ob_v.prepare(valid_bits, bitmap_bytes(len), mem, false, s)))
		return rc;
	if ((rc = ob_s.prepare(strand_bits, len * 8, mem, false, s)))
		return rc;
	SeqArgs a;
	memset(&a, 0, sizeof a);
	a.seq = v.d_seq;
	a.len = len;
	a.layout = v.lay;
	a.hp = hp;
	fill_mod(a.mod, 8, 0, 8);
	a.hashes = static_cast<uint64_t*>(ob_h.d);
	a.valid_bits = static_cast<uint8_t*>(ob_v.d);
	a.strand_bits = static_cast<uint64_t*>(ob_s.d);
	HIP_TRY(launch_seq_op(OP_HASH_ONLY, a, s));
	if ((rc = ob_h.finish(s)) || (rc = ob_v.finish(s)) || (rc = ob_s.finish(s)))
		return rc;
	HIP_TRY(hipStreamSynchronize(s)); // tables are freed on return
	return BTLBF_OK;
}
