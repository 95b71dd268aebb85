// csrc/host_mibf_fastx.cpp -- read classification from FASTA / FASTQ files (btlbf_mibf_classify_fastx_*), and the C entry
// points of its two device helpers (mibf_stream_kernels.hip).  The contracts are in include/btlbf.h.
//
// One sequential parser per file, each on a thread of its own (at most two; rows must come out in file order, so the
// byte-range readers of run_fastx, which deliver in arrival order, are not used), filling the parser's two pinned
// batches ahead of the caller.  btlbf_mibf_classify_fastx_next takes the next batch -- for two files the next run of
// pairs the zipper of mibf_zip.hpp forms from the two sides' current batches --, copies it to the device on the copy
// stream and runs, on the compute stream: interleave_mates (two files), btlbf_mibf_classify_seqs / _pairs with
// BTLBF_DEVICE, the tally kernel into the handle's running totals, and the copy of the four result arrays into one of
// two pinned result sets.  btlbf_mibf_classify_* plans its batches on the host and synchronises its stream, so `next`
// returns with batch j finished; what overlaps the GPU is the parsing of batches j + 1 and j + 2 on the parser threads.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"
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

namespace {

double now_s()
{
	using namespace std::chrono;
	return duration<double>(steady_clock::now().time_since_epoch()).count();
}

// a memory space's view of the arrays of a HOST-mode helper call: staged in, and the outputs copied back
struct Staged {
	DevBuf buf;
	void* host = nullptr;
	size_t n = 0;
	void* d = nullptr;
	int in(const void* user, size_t nbytes, int mem, bool copy, hipStream_t s)
	{
		n = nbytes;
		if (mem == BTLBF_DEVICE) {
			d = const_cast<void*>(user);
			return BTLBF_OK;
		}
		host = const_cast<void*>(user);
		HIP_TRY(buf.alloc_pooled(nbytes));
		d = buf.p;
		if (copy && nbytes)
			HIP_TRY(hipMemcpyAsync(d, user, nbytes, hipMemcpyHostToDevice, s));
		return BTLBF_OK;
	}
	int out(hipStream_t s)
	{
		if (host && n)
			HIP_TRY(hipMemcpyAsync(host, d, n, hipMemcpyDeviceToHost, s));
		return BTLBF_OK;
	}
};

} // namespace

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
	Staged a, sa, b, sb, o, so;
	int rc;
	if ((rc = a.in(seq1, starts1[n_pairs], mem, true, s)) || (rc = sa.in(starts1, (n_pairs + 1) * 8, mem, true, s)) ||
	    (rc = b.in(seq2, starts2[n_pairs], mem, true, s)) || (rc = sb.in(starts2, (n_pairs + 1) * 8, mem, true, s)) ||
	    (rc = o.in(out, starts1[0] + starts2[0] + n1 + n2, mem, false, s)) ||
	    (rc = so.in(out_starts, (2 * n_pairs + 1) * 8, mem, false, s)))
		return rc;
	HIP_TRY(launch_interleave_mates(static_cast<const uint8_t*>(a.d), static_cast<const uint64_t*>(sa.d),
	                                static_cast<const uint8_t*>(b.d), static_cast<const uint64_t*>(sb.d), n_pairs,
	                                static_cast<uint8_t*>(o.d), static_cast<uint64_t*>(so.d), s));
	if ((rc = o.out(s)) || (rc = so.out(s)))
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
	Staged h, n, sa, ev, b, a, t;
	int rc;
	if ((rc = h.in(hits, n_rows * max_results * sizeof(btlbf_mibf_hit), mem, true, s)) ||
	    (rc = n.in(n_hits, n_rows * 4, mem, true, s)) || (rc = sa.in(sat_count, n_rows * 4, mem, true, s)) ||
	    (rc = ev.in(eval_count, n_rows * 4, mem, true, s)) || (rc = b.in(best, n_ids * 8, mem, true, s)) ||
	    (rc = a.in(any, n_ids * 8, mem, true, s)) || (rc = t.in(totals6, 6 * 8, mem, true, s)))
		return rc;
	HIP_TRY(launch_mibf_tally(h.d, static_cast<const uint32_t*>(n.d), static_cast<const uint32_t*>(sa.d),
	                          static_cast<const uint32_t*>(ev.d), n_rows, max_results, n_ids,
	                          static_cast<unsigned long long*>(b.d), static_cast<unsigned long long*>(a.d),
	                          static_cast<unsigned long long*>(t.d), s));
	if (mem == BTLBF_DEVICE)
		return BTLBF_OK;
	if ((rc = b.out(s)) || (rc = a.out(s)) || (rc = t.out(s)))
		return rc;
	HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

// -------------------------------------------------------------------------------------------------
// the file classifier
// -------------------------------------------------------------------------------------------------
namespace {

struct HostBatch {
	const char* bases = nullptr;
	const uint64_t* starts = nullptr;
	uint64_t nb = 0, ns = 0; // ns == 0: end of input
};

// one file: its sequential parser on a thread of its own, at most two batches ahead of the consumer (the parser's two
// buffers: one batch is handed back, by release(), before the parser may overwrite it)
struct Side {
	btlbf_fastx* r = nullptr;
	std::thread th;
	std::mutex mu;
	std::condition_variable cv;
	std::deque<HostBatch> q;
	int credits = 2;
	bool abort = false;
	int rc = BTLBF_OK;
	std::string err;
	double seconds_parse = 0;
	bool holding = false; // the consumer has a batch of this side

	void run()
	{
		for (;;) {
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return credits > 0 || abort; });
				if (abort)
					return;
				--credits;
			}
			HostBatch b;
			const double t0 = now_s();
			const int e = btlbf_fastx_next(r, &b.bases, &b.nb, &b.starts, &b.ns);
			{
				std::lock_guard<std::mutex> lk(mu);
				seconds_parse += now_s() - t0;
				if (e) {
					rc = e;
					err = btlbf_last_error();
					b = HostBatch();
				}
				q.push_back(b);
			}
			cv.notify_all();
			if (e || b.ns == 0)
				return;
		}
	}
	// the next batch (ns == 0 at the end of input, and from then on); the one taken before goes back to the parser
	int take(HostBatch* out)
	{
		std::unique_lock<std::mutex> lk(mu);
		if (holding) {
			holding = false;
			++credits;
			cv.notify_all();
		}
		cv.wait(lk, [&] { return !q.empty(); });
		*out = q.front();
		if (rc && out->ns == 0)
			return btlbf_set_error(rc, "%s", err.c_str());
		if (out->ns) {
			q.pop_front();
			holding = true;
		}
		return BTLBF_OK;
	}
	void stop()
	{
		{
			std::lock_guard<std::mutex> lk(mu);
			abort = true;
		}
		cv.notify_all();
		if (th.joinable())
			th.join();
		if (r)
			btlbf_fastx_close(r);
		r = nullptr;
	}
};

// pinned or device memory that only grows
struct Grow {
	void* p = nullptr;
	uint64_t bytes = 0;
	bool pinned = false;
	hipError_t need(uint64_t n)
	{
		if (n <= bytes)
			return hipSuccess;
		release();
		n += n / 4;
		const hipError_t e = pinned ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
		if (e == hipSuccess)
			bytes = n;
		else
			p = nullptr;
		return e;
	}
	void release()
	{
		if (p)
			(void)(pinned ? hipHostFree(p) : hipFree(p));
		p = nullptr;
		bytes = 0;
	}
	template <class T>
	T* as() const
	{
		return static_cast<T*>(p);
	}
};

} // namespace

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
	// device: the tables, the batch (bases and starts per side, the interleaved buffer), the results, the totals
	double* d_prob = nullptr;
	uint32_t* d_minc = nullptr;
	Grow d_bases[2], d_starts[2], d_out, d_out_starts, d_hits, d_n, d_sat, d_eval;
	unsigned long long* d_tot = nullptr; // best[n_ids], any[n_ids], totals[6]
	// pinned: starts rebased to the batch, the rest of an odd interleaved batch, two result sets
	Grow h_starts[2], h_left, h_hits[2], h_n[2], h_sat[2], h_eval[2];
	uint64_t left_len = 0;
	bool has_left = false;
	int res = 0;
	uint64_t next_row = 0;
	bool ended = false;
	int end_rc = BTLBF_OK; // what the call that reached the end returned, and every later call returns
	std::string end_err;
	uint64_t n_batches = 0, n_bases = 0;

	btlbf_mibf_fastx()
	{
		for (Grow* g : {&h_starts[0], &h_starts[1], &h_left, &h_hits[0], &h_hits[1], &h_n[0], &h_n[1], &h_sat[0], &h_sat[1],
		                &h_eval[0], &h_eval[1]})
			g->pinned = true;
	}
	~btlbf_mibf_fastx()
	{
		side[0].stop();
		side[1].stop();
		if (comp_s)
			(void)hipStreamSynchronize(comp_s);
		if (copy_s)
			(void)hipStreamSynchronize(copy_s);
		for (Grow* g : {&d_bases[0], &d_bases[1], &d_starts[0], &d_starts[1], &d_out, &d_out_starts, &d_hits, &d_n, &d_sat,
		                &d_eval, &h_starts[0], &h_starts[1], &h_left, &h_hits[0], &h_hits[1], &h_n[0], &h_n[1], &h_sat[0],
		                &h_sat[1], &h_eval[0], &h_eval[1]})
			g->release();
		(void)hipFree(d_prob);
		(void)hipFree(d_minc);
		(void)hipFree(d_tot);
		if (copy_s)
			(void)hipStreamDestroy(copy_s);
		if (comp_s)
			(void)hipStreamDestroy(comp_s);
	}
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

// One batch on the device: n_rows rows over the sequences of `seq` (layout `starts`, n_seqs sequences): classify, tally,
// and -- for a caller who wants rows -- the copies into the pinned result set `c->res`
int run_batch(btlbf_mibf_fastx* c, const char* seq, uint64_t len, const uint64_t* starts, uint64_t n_seqs, uint64_t n_rows,
              bool want_rows)
{
	const uint64_t mr = c->par.max_results;
	if (c->d_hits.need(n_rows * mr * sizeof(btlbf_mibf_hit)) || c->d_n.need(n_rows * 4) || c->d_sat.need(n_rows * 4) ||
	    c->d_eval.need(n_rows * 4)) {
		(void)hipGetLastError();
		return fail(BTLBF_ENOMEM, "miBF classify file: results of %llu rows", (unsigned long long)n_rows);
	}
	btlbf_layout lay;
	lay.starts = starts;
	lay.n_seqs = n_seqs;
	lay.read_len = 0;
	const int rc = (c->pairs ? btlbf_mibf_classify_pairs : btlbf_mibf_classify_seqs)(
	    c->m, seq, len, &lay, &c->par, c->d_prob, c->d_minc, c->n_ids, c->d_hits.as<btlbf_mibf_hit>(), c->d_n.as<uint32_t>(),
	    c->d_sat.as<uint32_t>(), c->d_eval.as<uint32_t>(), BTLBF_DEVICE, c->comp_s);
	if (rc)
		return rc;
	HIP_TRY(launch_mibf_tally(c->d_hits.p, c->d_n.as<uint32_t>(), c->d_sat.as<uint32_t>(), c->d_eval.as<uint32_t>(), n_rows,
	                          c->par.max_results, c->n_ids, c->d_tot, c->d_tot + c->n_ids, c->d_tot + 2 * c->n_ids,
	                          c->comp_s));
	if (want_rows) {
		const int s = c->res;
		if (c->h_hits[s].need(n_rows * mr * sizeof(btlbf_mibf_hit)) || c->h_n[s].need(n_rows * 4) ||
		    c->h_sat[s].need(n_rows * 4) || c->h_eval[s].need(n_rows * 4)) {
			(void)hipGetLastError();
			return fail(BTLBF_ENOMEM, "miBF classify file: pinned results of %llu rows", (unsigned long long)n_rows);
		}
		HIP_TRY(hipMemcpyAsync(c->h_hits[s].p, c->d_hits.p, n_rows * mr * sizeof(btlbf_mibf_hit), hipMemcpyDeviceToHost,
		                       c->comp_s));
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
	if (c->d_bases[sd].need(lead_len + len + 64) || c->d_starts[sd].need((n + extra + 1) * 8) ||
	    c->h_starts[sd].need((n + extra + 1) * 8)) {
		(void)hipGetLastError();
		return fail(BTLBF_ENOMEM, "miBF classify file: a batch of %llu bytes", (unsigned long long)(lead_len + len));
	}
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
		if (c->d_out.need(l0 + l1 + 64) || c->d_out_starts.need((2 * n + 1) * 8)) {
			(void)hipGetLastError();
			return fail(BTLBF_ENOMEM, "miBF classify file: a batch of %llu bytes", (unsigned long long)(l0 + l1));
		}
		// the batch is on the device before the compute stream reads it (classify reads the offsets back on the host, too)
		HIP_TRY(hipStreamSynchronize(c->copy_s));
		HIP_TRY(launch_interleave_mates(c->d_bases[0].as<uint8_t>(), c->d_starts[0].as<uint64_t>(), c->d_bases[1].as<uint8_t>(),
		                                c->d_starts[1].as<uint64_t>(), n, c->d_out.as<uint8_t>(),
		                                c->d_out_starts.as<uint64_t>(), c->comp_s));
		HIP_TRY(hipStreamSynchronize(c->comp_s));
		if ((rc = run_batch(c, c->d_out.as<char>(), l0 + l1, c->d_out_starts.as<uint64_t>(), 2 * n, n, want_rows)))
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
			if (c->h_left.need(ll + 64)) {
				(void)hipGetLastError();
				return fail(BTLBF_ENOMEM, "miBF classify file: a record of %llu bytes", (unsigned long long)ll);
			}
			memcpy(c->h_left.p, b.bases + l0, ll);
			c->left_len = ll;
			c->has_left = true;
		}
		const uint64_t rows = c->pairs ? n_seqs / 2 : n_seqs;
		if (rows == 0)
			continue; // a batch of one record that waits for its mate
		if ((rc = run_batch(c, c->d_bases[0].as<char>(), len, c->d_starts[0].as<uint64_t>(), n_seqs, rows, want_rows)))
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
	hipError_t e = hipSuccess;
	// the parsers' pinned buffers need the device to be current
	if ((rc = btlbf_fastx_open(&c->side[0].r, path1, pf, k, c->cap)) ||
	    (path2 && (rc = btlbf_fastx_open(&c->side[1].r, path2, pf, k, c->cap))))
		goto bad;
	if ((e = hipStreamCreateWithFlags(&c->copy_s, hipStreamNonBlocking)) != hipSuccess ||
	    (e = hipStreamCreateWithFlags(&c->comp_s, hipStreamNonBlocking)) != hipSuccess ||
	    (e = hipMalloc(reinterpret_cast<void**>(&c->d_prob), n_ids * 8)) != hipSuccess ||
	    (e = hipMalloc(reinterpret_cast<void**>(&c->d_minc), n_ids * 4)) != hipSuccess ||
	    (e = hipMalloc(reinterpret_cast<void**>(&c->d_tot), (2 * n_ids + 6) * 8)) != hipSuccess ||
	    (e = hipMemcpy(c->d_prob, per_frame_prob, n_ids * 8, hipMemcpyHostToDevice)) != hipSuccess ||
	    (e = hipMemcpy(c->d_minc, min_count_per_id, n_ids * 4, hipMemcpyHostToDevice)) != hipSuccess ||
	    (e = hipMemset(c->d_tot, 0, (2 * n_ids + 6) * 8)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
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
	HIP_TRY(hipMemcpy(best, c->d_tot, c->n_ids * 8, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(any, c->d_tot + c->n_ids, c->n_ids * 8, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(totals6, c->d_tot + 2 * c->n_ids, 6 * 8, hipMemcpyDeviceToHost));
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
