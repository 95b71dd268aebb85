// csrc/host_mibf_fastx.cpp -- read classification from FASTA / FASTQ files (btlbf_mibf_classify_fastx_*), and the C entry
// points of its two device helpers (mibf_stream_kernels.hip).  The contracts are in include/btlbf.h.
//
// One sequential parser per file, each on a thread of its own (at most two; rows must come out in file order, so the
// byte-range readers of run_fastx, which deliver in arrival order, are not used), filling the parser's two pinned
// batches ahead of the caller.  btlbf_mibf_classify_fastx_next takes the next batch -- for two files the next run of
// pairs the zipper of mibf_zip.hpp forms from the two sides' current batches --, copies it to the device on the copy
// stream and runs, on the compute stream: interleave_mates (two files), mibf_classify_device (host_mibf.cpp) with the
// batch's host offsets (those stage_side wrote; for two files their closed form, mibf_zip_starts) and the handle's own
// scratch, the tally kernel into the handle's running totals, and the copy of the four result arrays into one of two
// pinned result sets.  mibf_classify_device plans its batches on the host and synchronises its stream, so `next` returns
// with batch j finished; what overlaps the GPU is the parsing of batches j + 1 and j + 2 on the parser threads.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"
#include "fastx_side.hpp"
#include "mibf_zip.hpp"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

using namespace btlbf;

extern "C" int btlbf_interleave_mates(const char* seq1, const uint64_t* starts1, const char* seq2, const uint64_t* starts2,
                                      uint64_t n_pairs, char* out, uint64_t* out_starts, int mem, int device, void* stream)
{
	if (!starts1 || !starts2 || !out_starts) // seq1, seq2 and out may hold no byte
		return btlbf_set_error(BTLBF_EINVAL, "null argument");
	DeviceGuard g(device);
	if (!g.ok)
		return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (mem == BTLBF_DEVICE) {
		HIP_TRY(launch_interleave_mates(reinterpret_cast<const uint8_t*>(seq1), starts1, reinterpret_cast<const uint8_t*>(seq2),
		                                starts2, n_pairs, reinterpret_cast<uint8_t*>(out), out_starts, s));
		return BTLBF_OK;
	}
	const uint64_t n1 = starts1[n_pairs] - starts1[0], n2 = starts2[n_pairs] - starts2[0];
	for (uint64_t i = 0; i < n_pairs; ++i)
		if (starts1[i + 1] < starts1[i] || starts2[i + 1] < starts2[i])
			return btlbf_set_error(BTLBF_EINVAL, "starts must not decrease");
	InBuf a, sa, b, sb;
	OutBuf o, so;
	int rc;
	if ((rc = a.prepare(seq1, starts1[n_pairs], mem, s)) || (rc = sa.prepare(starts1, (n_pairs + 1) * 8, mem, s)) ||
	    (rc = b.prepare(seq2, starts2[n_pairs], mem, s)) || (rc = sb.prepare(starts2, (n_pairs + 1) * 8, mem, s)) ||
	    (rc = o.prepare(out, starts1[0] + starts2[0] + n1 + n2, mem, false, s)) ||
	    (rc = so.prepare(out_starts, (2 * n_pairs + 1) * 8, mem, false, s)))
		return rc;
	HIP_TRY(launch_interleave_mates(a.as<uint8_t>(), sa.as<uint64_t>(), b.as<uint8_t>(), sb.as<uint64_t>(), n_pairs,
	                                o.as<uint8_t>(), so.as<uint64_t>(), s));
	if ((rc = o.finish(s)) || (rc = so.finish(s)))
		return rc;
	HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_classify_tally(const btlbf_mibf_hit* hits, const uint32_t* n_hits, const uint32_t* sat_count,
                                         const uint32_t* eval_count, uint64_t n_rows, uint32_t max_results, uint64_t n_ids,
                                         uint64_t* best, uint64_t* any, uint64_t* totals6, int mem, int device, void* stream)
{
	if ((n_rows && (!hits || !n_hits || !sat_count || !eval_count)) || !best || !any || !totals6)
		return btlbf_set_error(BTLBF_EINVAL, "null argument");
	if (max_results == 0 || n_ids == 0)
		return btlbf_set_error(BTLBF_EINVAL, "miBF tally: max_results and n_ids must be at least 1");
	DeviceGuard g(device);
	if (!g.ok)
		return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	InBuf h, n, sa, ev;
	OutBuf b, a, t; // updated: the caller's counts go in first
	int rc;
	if ((rc = h.prepare(hits, n_rows * max_results * sizeof(btlbf_mibf_hit), mem, s)) ||
	    (rc = n.prepare(n_hits, n_rows * 4, mem, s)) || (rc = sa.prepare(sat_count, n_rows * 4, mem, s)) ||
	    (rc = ev.prepare(eval_count, n_rows * 4, mem, s)) || (rc = b.prepare(best, n_ids * 8, mem, false, s, true)) ||
	    (rc = a.prepare(any, n_ids * 8, mem, false, s, true)) || (rc = t.prepare(totals6, 6 * 8, mem, false, s, true)))
		return rc;
	HIP_TRY(launch_mibf_tally(h.as<void>(), n.as<uint32_t>(), sa.as<uint32_t>(), ev.as<uint32_t>(), n_rows, max_results, n_ids,
	                          b.as<unsigned long long>(), a.as<unsigned long long>(), t.as<unsigned long long>(), s));
	if (mem == BTLBF_DEVICE)
		return BTLBF_OK;
	if ((rc = b.finish(s)) || (rc = a.finish(s)) || (rc = t.finish(s)))
		return rc;
	HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

// -------------------------------------------------------------------------------------------------
// the file classifier (a file and its parser thread: Side, fastx_side.hpp)
// -------------------------------------------------------------------------------------------------
struct btlbf_mibf_fastx {
	btlbf_mibf* m = nullptr;
	int device = 0;
	bool pairs = false, two_files = false;
	btlbf_mibf_classify_params par{};
	uint64_t n_ids = 0, cap = 0;
	Side side[2];
	MibfZip zip;
	HostBatch cur[2];
	hipStream_t copy_s = nullptr, comp_s = nullptr;
	// grow only, free themselves.  Device: the tables, the totals (best[n_ids], any[n_ids], totals[6]), the batch (bases and
	// starts per side, the interleaved buffer), the results; pinned: the sides' starts, an odd batch's rest, two result sets
	DevScratch d_prob, d_minc, d_tot, d_bases[2], d_starts[2], d_out, d_out_starts, d_hits, d_n, d_sat, d_eval;
	PinScratch h_starts[2], h_left, h_hits[2], h_n[2], h_sat[2], h_eval[2];
	MibfClassifyScratch scratch;
	MibfSeqs seqs; // the batch's sequences for the planner: the host offsets
	uint64_t left_len = 0;
	bool has_left = false;
	int res = 0;
	uint64_t next_row = 0;
	bool ended = false;
	int end_rc = BTLBF_OK; // what the call that reached the end returned, and every later call returns
	std::string end_err;
	uint64_t n_batches = 0, n_bases = 0;

	btlbf_mibf_fastx() { scratch.kept = true; }
	~btlbf_mibf_fastx() // the buffers go after this: none while work is pending
	{
		side[0].stop();
		side[1].stop();
		for (hipStream_t s : {comp_s, copy_s})
			if (s) {
				(void)hipStreamSynchronize(s);
				(void)hipStreamDestroy(s);
			}
	}
	template <class Buf>
	bool room(Buf& b, uint64_t n) { return b.keep_room(n, device); }
	unsigned long long* tot() const { return d_tot.as<unsigned long long>(); }
};

namespace {

int file_readable(const char* path)
{
	FILE* fp = fopen(path, "rb");
	if (!fp)
		return btlbf_set_error(BTLBF_EIO, "file \"%s\" could not be read.", path);
	fclose(fp);
	return BTLBF_OK;
}

int end_input(btlbf_mibf_fastx* c, int rc)
{
	c->ended = true;
	c->end_rc = rc;
	c->end_err = rc ? btlbf_last_error() : "";
	return rc;
}

// One batch on the device: n_rows rows over the sequences of d_seq[0, len), whose offsets are c->seqs.starts and, on the
// device, d_starts: classify, tally, and -- for a caller who wants rows -- the copies into the pinned result set `c->res`
int run_batch(btlbf_mibf_fastx* c, const void* d_seq, uint64_t len, const void* d_starts, uint64_t n_rows, bool want_rows)
{
	const uint64_t hit_bytes = n_rows * c->par.max_results * sizeof(btlbf_mibf_hit);
	c->seqs.n_seqs = c->seqs.starts.size() - 1;
	if (!c->room(c->d_hits, hit_bytes) || !c->room(c->d_n, n_rows * 4) || !c->room(c->d_sat, n_rows * 4) ||
	    !c->room(c->d_eval, n_rows * 4))
		return fail(BTLBF_ENOMEM, "miBF classify file: results of %llu rows", (unsigned long long)n_rows);
	const int rc = mibf_classify_device(c->m, static_cast<const uint8_t*>(d_seq), len, c->seqs,
	                                    static_cast<const uint64_t*>(d_starts), c->par, c->d_prob.as<double>(),
	                                    c->d_minc.as<uint32_t>(), c->n_ids, c->d_hits.as<btlbf_mibf_hit>(),
	                                    c->d_n.as<uint32_t>(), c->d_sat.as<uint32_t>(), c->d_eval.as<uint32_t>(), c->pairs,
	                                    c->comp_s, c->scratch);
	if (rc)
		return rc;
	HIP_TRY(launch_mibf_tally(c->d_hits.p, c->d_n.as<uint32_t>(), c->d_sat.as<uint32_t>(), c->d_eval.as<uint32_t>(), n_rows,
	                          c->par.max_results, c->n_ids, c->tot(), c->tot() + c->n_ids, c->tot() + 2 * c->n_ids, c->comp_s));
	if (want_rows) {
		const int s = c->res;
		if (!c->room(c->h_hits[s], hit_bytes) || !c->room(c->h_n[s], n_rows * 4) || !c->room(c->h_sat[s], n_rows * 4) ||
		    !c->room(c->h_eval[s], n_rows * 4))
			return fail(BTLBF_ENOMEM, "miBF classify file: pinned results of %llu rows", (unsigned long long)n_rows);
		HIP_TRY(hipMemcpyAsync(c->h_hits[s].p, c->d_hits.p, hit_bytes, hipMemcpyDeviceToHost, c->comp_s));
		HIP_TRY(hipMemcpyAsync(c->h_n[s].p, c->d_n.p, n_rows * 4, hipMemcpyDeviceToHost, c->comp_s));
		HIP_TRY(hipMemcpyAsync(c->h_sat[s].p, c->d_sat.p, n_rows * 4, hipMemcpyDeviceToHost, c->comp_s));
		HIP_TRY(hipMemcpyAsync(c->h_eval[s].p, c->d_eval.p, n_rows * 4, hipMemcpyDeviceToHost, c->comp_s));
	}
	HIP_TRY(hipStreamSynchronize(c->comp_s));
	++c->n_batches;
	c->n_bases += len;
	return BTLBF_OK;
}

// records [a, a + n) of a parsed batch onto the device as side `sd` of the batch: the bases and the n + 1 offsets,
// rebased to the first record.  With `lead` (an interleaved file: the record the batch before left over, lead_len bytes
// of c->h_left) that record comes first, and the offsets have an entry for it
int stage_side(btlbf_mibf_fastx* c, int sd, const HostBatch& b, uint64_t a, uint64_t n, bool lead, uint64_t lead_len,
               uint64_t* len_out)
{
	const uint64_t b0 = b.starts[a], len = b.starts[a + n] - b0, extra = lead ? 1 : 0;
	if (!c->room(c->d_bases[sd], lead_len + len + 64) || !c->room(c->d_starts[sd], (n + extra + 1) * 8) ||
	    !c->room(c->h_starts[sd], (n + extra + 1) * 8))
		return fail(BTLBF_ENOMEM, "miBF classify file: a batch of %llu bytes", (unsigned long long)(lead_len + len));
	uint64_t* hs = c->h_starts[sd].as<uint64_t>();
	hs[0] = 0;
	for (uint64_t i = 0; i <= n; ++i)
		hs[extra + i] = lead_len + b.starts[a + i] - b0;
	if (lead_len)
		HIP_TRY(hipMemcpyAsync(c->d_bases[sd].p, c->h_left.p, lead_len, hipMemcpyHostToDevice, c->copy_s));
	if (len)
		HIP_TRY(hipMemcpyAsync(c->d_bases[sd].as<char>() + lead_len, b.bases + b0, len, hipMemcpyHostToDevice, c->copy_s));
	HIP_TRY(hipMemcpyAsync(c->d_starts[sd].p, hs, (n + extra + 1) * 8, hipMemcpyHostToDevice, c->copy_s));
	*len_out = lead_len + len;
	return BTLBF_OK;
}

// the next rows: *n_rows == 0 at the end of input
int next_rows(btlbf_mibf_fastx* c, uint64_t* n_rows, bool want_rows)
{
	*n_rows = 0;
	int rc;
	if (c->two_files) {
		for (;;) {
			const MibfZip::Step st = c->zip.step();
			if (st == MibfZip::END)
				return end_input(c, BTLBF_OK);
			if (st == MibfZip::UNEQUAL)
				return end_input(c, btlbf_set_error(BTLBF_EFORMAT, "miBF classify file: the two files do not pair up: one ends "
				                                    "after %llu records, the other goes on", (unsigned long long)c->zip.pairs));
			if (st == MibfZip::TAKE)
				break;
			const int sd = st == MibfZip::NEED_1;
			if ((rc = c->side[sd].take(&c->cur[sd])))
				return end_input(c, rc);
			c->zip.feed(sd, c->cur[sd].ns, c->cur[sd].ns == 0);
		}
		const uint64_t a0 = c->zip.pos(0), a1 = c->zip.pos(1), n = c->zip.take();
		uint64_t l0 = 0, l1 = 0;
		if ((rc = stage_side(c, 0, c->cur[0], a0, n, false, 0, &l0)) ||
		    (rc = stage_side(c, 1, c->cur[1], a1, n, false, 0, &l1)))
			return rc;
		if (!c->room(c->d_out, l0 + l1 + 64) || !c->room(c->d_out_starts, (2 * n + 1) * 8))
			return fail(BTLBF_ENOMEM, "miBF classify file: a batch of %llu bytes", (unsigned long long)(l0 + l1));
		HIP_TRY(hipStreamSynchronize(c->copy_s)); // the batch is on the device before the compute stream reads it
		// the kernels read the interleaved offsets on the device; the planner gets the same on the host
		HIP_TRY(launch_interleave_mates(c->d_bases[0].as<uint8_t>(), c->d_starts[0].as<uint64_t>(), c->d_bases[1].as<uint8_t>(),
		                                c->d_starts[1].as<uint64_t>(), n, c->d_out.as<uint8_t>(),
		                                c->d_out_starts.as<uint64_t>(), c->comp_s));
		c->seqs.starts = mibf_zip_starts(c->h_starts[0].as<uint64_t>(), c->h_starts[1].as<uint64_t>(), n);
		if ((rc = run_batch(c, c->d_out.p, l0 + l1, c->d_out_starts.p, n, want_rows)))
			return rc;
		*n_rows = n;
		return BTLBF_OK;
	}
	for (;;) {
		HostBatch& b = c->cur[0];
		if ((rc = c->side[0].take(&b)))
			return end_input(c, rc);
		if (b.ns == 0) {
			if (c->has_left)
				return end_input(c, btlbf_set_error(BTLBF_EFORMAT, "miBF classify file: an interleaved file of %llu records: "
				                                    "the last one has no mate", (unsigned long long)(2 * c->next_row + 1)));
			return end_input(c, BTLBF_OK);
		}
		// interleaved: the record an odd batch left over leads this one, and an odd total leaves its last record over
		const bool led = c->has_left;
		const uint64_t total = b.ns + (led ? 1 : 0);
		const bool odd = c->pairs && (total & 1);
		const uint64_t n = odd ? b.ns - 1 : b.ns;
		uint64_t len = 0;
		if ((rc = stage_side(c, 0, b, 0, n, led, led ? c->left_len : 0, &len)))
			return rc;
		HIP_TRY(hipStreamSynchronize(c->copy_s)); // also: h_left may be written again below
		const uint64_t n_seqs = n + (led ? 1 : 0);
		c->has_left = false;
		if (odd) {
			const uint64_t l0 = b.starts[b.ns - 1], ll = b.starts[b.ns] - l0;
			if (!c->room(c->h_left, ll + 64))
				return fail(BTLBF_ENOMEM, "miBF classify file: a record of %llu bytes", (unsigned long long)ll);
			memcpy(c->h_left.p, b.bases + l0, ll);
			c->left_len = ll;
			c->has_left = true;
		}
		const uint64_t rows = c->pairs ? n_seqs / 2 : n_seqs;
		if (rows == 0)
			continue; // a batch of one record that waits for its mate
		c->seqs.starts.assign(c->h_starts[0].as<uint64_t>(), c->h_starts[0].as<uint64_t>() + n_seqs + 1);
		if ((rc = run_batch(c, c->d_bases[0].p, len, c->d_starts[0].p, rows, want_rows)))
			return rc;
		*n_rows = rows;
		return BTLBF_OK;
	}
}

} // namespace

extern "C" int btlbf_mibf_classify_fastx_open(btlbf_mibf_fastx** out, btlbf_mibf* m, const char* path1, const char* path2,
                                              uint32_t flags, const btlbf_mibf_classify_params* p,
                                              const double* per_frame_prob, const uint32_t* min_count_per_id, uint64_t n_ids,
                                              uint64_t batch_bytes)
{
	if (!out || !m || !path1 || !p || !per_frame_prob || !min_count_per_id)
		return btlbf_set_error(BTLBF_EINVAL, "null argument");
	*out = nullptr;
	if (p->max_results == 0)
		return btlbf_set_error(BTLBF_EINVAL, "miBF classify file: max_results must be at least 1");
	if (n_ids == 0)
		return btlbf_set_error(BTLBF_EINVAL, "miBF classify file: n_ids must be at least 1");
	if (path2 && (flags & BTLBF_CLASSIFY_INTERLEAVED))
		return btlbf_set_error(BTLBF_EINVAL, "miBF classify file: mates come from a second file or from an interleaved "
		                       "file (BTLBF_CLASSIFY_INTERLEAVED), not both");
	int rc;
	if ((rc = file_readable(path1)) || (path2 && (rc = file_readable(path2))))
		return rc;
	const unsigned id_bytes = mibf_id_bytes(m);
	if (n_ids > (1ull << (id_bytes * 8 - 1)))
		return btlbf_set_error(BTLBF_EINVAL, "miBF classify file: n_ids must be 1..2^%u for %u-byte ids, not %llu",
		                       id_bytes * 8 - 1, id_bytes, (unsigned long long)n_ids);
	btlbf_mibf_fastx* c = new (std::nothrow) btlbf_mibf_fastx;
	if (!c)
		return btlbf_set_error(BTLBF_ENOMEM, "miBF classify file: out of memory");
	c->m = m;
	c->device = mibf_device(m);
	c->two_files = path2 != nullptr;
	c->pairs = c->two_files || (flags & BTLBF_CLASSIFY_INTERLEAVED);
	c->par = *p;
	c->n_ids = n_ids;
	c->cap = batch_bytes ? batch_bytes : 64ull << 20;
	DeviceGuard g(c->device);
	const uint32_t pf = (flags & (BTLBF_FASTX_LINES | BTLBF_FASTX_PAGEABLE)) | BTLBF_FASTX_WHOLE;
	const uint32_t k = btlbf_mibf_kmer_size(m);
	const uint64_t tot_bytes = (2 * n_ids + 6) * 8;
	hipError_t e = hipSuccess;
	// the parsers' pinned buffers need the device to be current
	if ((rc = btlbf_fastx_open(&c->side[0].r, path1, pf, k, c->cap)) ||
	    (path2 && (rc = btlbf_fastx_open(&c->side[1].r, path2, pf, k, c->cap))))
		goto bad;
	if (!c->d_prob.grow(n_ids * 8, c->device) || !c->d_minc.grow(n_ids * 4, c->device) || !c->d_tot.grow(tot_bytes, c->device))
		e = hipErrorOutOfMemory;
	if (e != hipSuccess || (e = hipStreamCreateWithFlags(&c->copy_s, hipStreamNonBlocking)) != hipSuccess ||
	    (e = hipStreamCreateWithFlags(&c->comp_s, hipStreamNonBlocking)) != hipSuccess ||
	    (e = hipMemcpy(c->d_prob.p, per_frame_prob, n_ids * 8, hipMemcpyHostToDevice)) != hipSuccess ||
	    (e = hipMemcpy(c->d_minc.p, min_count_per_id, n_ids * 4, hipMemcpyHostToDevice)) != hipSuccess ||
	    (e = hipMemset(c->d_tot.p, 0, tot_bytes)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
		rc = fail(BTLBF_EHIP, "miBF classify file: %s", hipGetErrorString(e));
		goto bad;
	}
	for (int s = 0; s < (c->two_files ? 2 : 1); ++s)
		c->side[s].th = std::thread([c, s] { c->side[s].run(); });
	*out = c;
	return BTLBF_OK;
bad:
	delete c;
	return rc;
}

extern "C" int btlbf_mibf_classify_fastx_next(btlbf_mibf_fastx* c, uint64_t* first_row, uint64_t* n_rows,
                                              const btlbf_mibf_hit** hits, const uint32_t** n_hits,
                                              const uint32_t** sat_count, const uint32_t** eval_count)
{
	if (!c || !first_row || !n_rows)
		return btlbf_set_error(BTLBF_EINVAL, "null argument");
	const bool want_rows = hits || n_hits || sat_count || eval_count;
	if (want_rows && (!hits || !n_hits || !sat_count || !eval_count))
		return btlbf_set_error(BTLBF_EINVAL, "miBF classify file: the four result pointers are given together or not at all");
	*first_row = c->next_row;
	*n_rows = 0;
	if (c->ended)
		return c->end_rc ? btlbf_set_error(c->end_rc, "%s", c->end_err.c_str()) : BTLBF_OK;
	DeviceGuard g(c->device);
	c->res ^= 1;
	uint64_t n = 0;
	const int rc = next_rows(c, &n, want_rows);
	if (rc)
		return rc;
	*n_rows = n;
	c->next_row += n;
	if (want_rows) {
		*hits = n ? c->h_hits[c->res].as<btlbf_mibf_hit>() : nullptr;
		*n_hits = n ? c->h_n[c->res].as<uint32_t>() : nullptr;
		*sat_count = n ? c->h_sat[c->res].as<uint32_t>() : nullptr;
		*eval_count = n ? c->h_eval[c->res].as<uint32_t>() : nullptr;
	}
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_classify_fastx_tally(btlbf_mibf_fastx* c, uint64_t* best, uint64_t* any, uint64_t* totals6)
{
	if (!c || !best || !any || !totals6)
		return btlbf_set_error(BTLBF_EINVAL, "null argument");
	DeviceGuard g(c->device);
	HIP_TRY(hipStreamSynchronize(c->comp_s));
	HIP_TRY(hipMemcpy(best, c->tot(), c->n_ids * 8, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(any, c->tot() + c->n_ids, c->n_ids * 8, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(totals6, c->tot() + 2 * c->n_ids, 6 * 8, hipMemcpyDeviceToHost));
	return BTLBF_OK;
}

extern "C" void btlbf_mibf_classify_fastx_close(btlbf_mibf_fastx* c)
{
	if (!c)
		return;
	DeviceGuard g(c->device);
	delete c;
}

extern "C" int btlbf_mibf_classify_fastx(btlbf_mibf* m, const char* path1, const char* path2, uint32_t flags,
                                         const btlbf_mibf_classify_params* p, const double* per_frame_prob,
                                         const uint32_t* min_count_per_id, uint64_t n_ids, uint64_t batch_bytes,
                                         uint64_t* best, uint64_t* any, uint64_t* totals6, btlbf_fastx_stats* stats)
{
	if (!best || !any || !totals6)
		return btlbf_set_error(BTLBF_EINVAL, "null argument");
	const double t0 = now_s();
	btlbf_mibf_fastx* c = nullptr;
	int rc = btlbf_mibf_classify_fastx_open(&c, m, path1, path2, flags, p, per_frame_prob, min_count_per_id, n_ids,
	                                        batch_bytes);
	if (rc)
		return rc;
	uint64_t first = 0, n = 0;
	do
		rc = btlbf_mibf_classify_fastx_next(c, &first, &n, nullptr, nullptr, nullptr, nullptr);
	while (rc == BTLBF_OK && n);
	if (rc == BTLBF_OK)
		rc = btlbf_mibf_classify_fastx_tally(c, best, any, totals6);
	if (stats) {
		memset(stats, 0, sizeof *stats);
		stats->n_batches = c->n_batches;
		stats->n_bases = c->n_bases;
		for (int s = 0; s < 2; ++s)
			if (c->side[s].r) {
				std::lock_guard<std::mutex> lk(c->side[s].mu);
				stats->n_records += btlbf_fastx_records(c->side[s].r);
				stats->seconds_parse = std::max(stats->seconds_parse, c->side[s].seconds_parse);
			}
	}
	std::string err = rc ? btlbf_last_error() : "";
	btlbf_mibf_classify_fastx_close(c);
	if (stats)
		stats->seconds_total = now_s() - t0;
	return rc ? btlbf_set_error(rc, "%s", err.c_str()) : BTLBF_OK;
}
