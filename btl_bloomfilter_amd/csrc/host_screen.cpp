// csrc/host_screen.cpp -- the read screen: btlbf_screen_seqs, btlbf_screen_tally and the file handle
// btlbf_screen_fastx_* (contracts: include/btlbf.h; kernels: screen_kernels.hip).
//
// A call checks its arguments without touching the filters, takes every filter's lock in ascending handle address,
// checks that the filters can share one hash stage, and runs screen_device: the filters in groups of at most
// kScreenMaxNF (screen_plan.hpp), each group one launch of the fused kernel that writes its hit columns -- and the first
// one the valid column -- of the per-window bitmaps; then one reduction of all columns to hits[row][filter] and
// valid[row], and the verdict.  The file handle feeds the same core from the ordered reader of fastx_side.hpp.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"
#include "fastx_side.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <string>

using namespace btlbf;

namespace {

// the filters of a call, in the caller's order (the columns) and in ascending address (the locks)
struct ScreenSet {
	unsigned n = 0;
	btlbf_filter* f[kScreenMaxFilters] = {nullptr};
	btlbf_filter* by_addr[kScreenMaxFilters] = {nullptr};
};

// what can be said without looking at a filter: before any HIP call, nothing dereferenced but the array itself
int check_set(ScreenSet& set, btlbf_filter* const* filters, unsigned n_filters, const btlbf_screen_params* p)
{
	if (!filters || !p)
		return btlbf_set_error(BTLBF_EINVAL, "screen: null argument");
	if (n_filters == 0 || n_filters > kScreenMaxFilters)
		return btlbf_set_error(BTLBF_EINVAL, "screen: n_filters must be 1..%u, not %u", kScreenMaxFilters, n_filters);
	if (!(p->min_fraction >= 0.0 && p->min_fraction <= 1.0)) // (a NaN compares false)
		return btlbf_set_error(BTLBF_EINVAL, "screen: min_fraction must be in [0, 1]");
	set.n = n_filters;
	for (unsigned j = 0; j < n_filters; ++j) {
		if (!filters[j])
			return btlbf_set_error(BTLBF_EINVAL, "screen: filter %u is a null handle", j);
		set.f[j] = set.by_addr[j] = filters[j];
	}
	std::sort(set.by_addr, set.by_addr + n_filters, std::less<btlbf_filter*>());
	for (unsigned j = 1; j < n_filters; ++j)
		if (set.by_addr[j] == set.by_addr[j - 1])
			return btlbf_set_error(BTLBF_EINVAL, "screen: the same handle twice");
	return BTLBF_OK;
}

struct SetLock {
	const ScreenSet* set = nullptr;
	void lock(const ScreenSet& s)
	{
		set = &s;
		for (unsigned j = 0; j < s.n; ++j)
			s.by_addr[j]->mu.lock();
	}
	~SetLock()
	{
		if (set)
			for (unsigned j = set->n; j-- > 0;)
				set->by_addr[j]->mu.unlock();
	}
};

// can the filters share one hash stage?  (under their locks; still no HIP call)
int check_compatible(const ScreenSet& set)
{
	const btlbf_filter* f0 = set.f[0];
	for (unsigned j = 0; j < set.n; ++j) {
		const btlbf_filter* f = set.f[j];
		if (f->kind != BTLBF_BLOOM)
			return btlbf_set_error(BTLBF_EINVAL, "screen: filter %u is not a bit filter (BTLBF_BLOOM): counting filters are "
			                       "not screened", j);
		if (f->shard_count != 1)
			return btlbf_set_error(BTLBF_EINVAL, "screen: filter %u is a shard", j);
		if (f->device != f0->device)
			return btlbf_set_error(BTLBF_EINVAL, "screen: filter %u is on device %d, filter 0 on device %d", j, f->device,
			                       f0->device);
		if (f->k != f0->k || f->h != f0->h)
			return btlbf_set_error(BTLBF_EINVAL, "screen: filter %u has kmer_size %u and hash_num %u, filter 0 has %u and %u",
			                       j, f->k, f->h, f0->k, f0->h);
		if (f->hp.n_seeds != f0->hp.n_seeds || f->hp.h2 != f0->hp.h2 || f->seed_strs != f0->seed_strs)
			return btlbf_set_error(BTLBF_EINVAL, "screen: filter %u and filter 0 differ in their spaced seeds", j);
	}
	if (f0->hp.n_seeds == 0 && f0->h > 64)
		return btlbf_set_error(BTLBF_EINVAL, "screen: hash_num %u > 64 unsupported by the sequence kernels", f0->h);
	return BTLBF_OK;
}

// The screen of d_seq[0, len) on the device: n_rows rows into d_hits[n_rows * n], d_valid, d_pass (may be null), queued
// on s.  The filters are locked and compatible, their device is current; `cols` holds the bitmaps until s has run.
int screen_device(const ScreenSet& set, const uint8_t* d_seq, uint64_t len, const LayoutParams& lay, uint64_t n_rows,
                  const btlbf_screen_params& p, uint32_t* d_hits, uint32_t* d_valid, uint32_t* d_pass, DevScratch& cols,
                  hipStream_t s)
{
	if (n_rows == 0)
		return BTLBF_OK;
	for (unsigned j = 0; j < set.n; ++j)
		MATERIALIZE(set.f[j], s);
	if (len == 0) { // rows without a byte
		HIP_TRY(hipMemsetAsync(d_hits, 0, n_rows * set.n * 4, s));
		HIP_TRY(hipMemsetAsync(d_valid, 0, n_rows * 4, s));
		if (d_pass)
			HIP_TRY(hipMemsetAsync(d_pass, 0, n_rows * 4, s));
		return BTLBF_OK;
	}
	const uint64_t col_bytes = screen_col_bytes(len);
	if (!cols.keep_room((set.n + 1) * col_bytes, set.f[0]->device))
		return fail(BTLBF_ENOMEM, "screen: %llu bytes of per-window bitmaps", (unsigned long long)((set.n + 1) * col_bytes));
	const ScreenGroups groups = screen_groups(set.n);
	for (unsigned g = 0; g < groups.n; ++g) {
		ScreenArgs a;
		memset(&a, 0, sizeof a);
		a.seq = d_seq;
		a.len = len;
		a.layout = lay;
		a.hp = set.f[0]->hp;
		a.nf = groups.size[g];
		for (unsigned j = 0; j < a.nf; ++j) {
			const btlbf_filter* f = set.f[groups.first[g] + j];
			REQUIRE_MATERIALIZED(f);
			a.words[j] = static_cast<const uint32_t*>(f->d_data);
			a.mod[j] = f->mod;
		}
		a.hit_cols = cols.as<uint8_t>() + groups.first[g] * col_bytes;
		a.col_bytes = col_bytes;
		a.valid_bits = g == 0 ? cols.as<uint8_t>() + set.n * col_bytes : nullptr;
		HIP_TRY(launch_screen(a, s));
	}
	HIP_TRY(launch_screen_reduce(cols.as<uint64_t>(), col_bytes / 8, len, lay, n_rows, set.f[0]->k, set.n, d_hits, d_valid, s));
	if (d_pass)
		HIP_TRY(launch_screen_verdict(d_hits, d_valid, n_rows, set.n, p.min_fraction, p.min_hits, d_pass, s));
	return BTLBF_OK;
}

} // namespace

extern "C" int btlbf_screen_seqs(btlbf_filter* const* filters, unsigned n_filters, const char* seq, uint64_t len,
                                 const btlbf_layout* layout, const btlbf_screen_params* p, uint32_t* hits, uint32_t* valid,
                                 uint32_t* pass_bits, int mem, void* stream)
{
	if (!hits || !valid || (len && !seq))
		return btlbf_set_error(BTLBF_EINVAL, "screen: null argument");
	ScreenSet set;
	int rc = check_set(set, filters, n_filters, p);
	if (rc)
		return rc;
	if (mem != BTLBF_HOST && mem != BTLBF_DEVICE)
		return btlbf_set_error(BTLBF_EINVAL, "mem must be BTLBF_HOST or BTLBF_DEVICE");
	const bool has_starts = layout && layout->starts;
	const uint32_t read_len = layout && !has_starts ? layout->read_len : 0;
	if (read_len && len % read_len)
		return btlbf_set_error(BTLBF_EINVAL, "len %llu is not a multiple of read_len %u", (unsigned long long)len, read_len);
	SetLock lk;
	lk.lock(set);
	if ((rc = check_compatible(set)))
		return rc;
	const uint64_t n_rows = screen_rows(has_starts, layout ? layout->n_seqs : 0, read_len, len);
	if (n_rows == 0)
		return BTLBF_OK;
	DeviceGuard g(set.f[0]->device);
	if (!g.ok)
		return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", set.f[0]->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	SeqView v;
	if ((rc = make_view(v, seq, len, layout, mem, s)))
		return rc;
	OutBuf ob_hits, ob_valid, ob_pass;
	if ((rc = ob_hits.prepare(hits, n_rows * n_filters * 4, mem, false, s)) ||
	    (rc = ob_valid.prepare(valid, n_rows * 4, mem, false, s)) || (rc = ob_pass.prepare(pass_bits, n_rows * 4, mem, false, s)))
		return rc;
	// The bitmaps: scratch of the filter with the lowest address, whose lock this call holds.  A BTLBF_DEVICE call returns
	// with its work queued, so the scratch is handed from call to call in stream order: this stream first waits for the
	// event the previous user recorded behind its last kernel, and records its own (freeing or growing the scratch
	// synchronises the device, GrowOnly::release)
	btlbf_filter* owner = set.by_addr[0];
	if (owner->screen_ev_pending)
		HIP_TRY(hipStreamWaitEvent(s, owner->screen_ev, 0));
	rc = screen_device(set, v.d_seq, len, v.lay, n_rows, *p, ob_hits.as<uint32_t>(), ob_valid.as<uint32_t>(),
	                   ob_pass.as<uint32_t>(), owner->screen, s);
	if (!owner->screen_ev && hipEventCreateWithFlags(&owner->screen_ev, hipEventDisableTiming) != hipSuccess) {
		(void)hipGetLastError();
		owner->screen_ev = nullptr;
	}
	if (owner->screen_ev && hipEventRecord(owner->screen_ev, s) == hipSuccess) {
		owner->screen_ev_pending = true;
	} else { // no event to hand the scratch on with: wait here
		(void)hipGetLastError();
		(void)hipStreamSynchronize(s);
		owner->screen_ev_pending = false;
	}
	if (rc)
		return rc;
	if ((rc = ob_hits.finish(s)) || (rc = ob_valid.finish(s)) || (rc = ob_pass.finish(s)))
		return rc;
	if (mem == BTLBF_HOST)
		HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

extern "C" int btlbf_screen_tally(const uint32_t* hits, const uint32_t* valid, const uint32_t* pass_bits, uint64_t n_rows,
                                  unsigned n_filters, uint64_t* passed, uint64_t* best, uint64_t* totals4, int mem, int device,
                                  void* stream)
{
	if ((n_rows && (!hits || !valid || !pass_bits)) || !passed || !best || !totals4)
		return btlbf_set_error(BTLBF_EINVAL, "screen tally: null argument");
	if (n_filters == 0 || n_filters > kScreenMaxFilters)
		return btlbf_set_error(BTLBF_EINVAL, "screen tally: n_filters must be 1..%u, not %u", kScreenMaxFilters, n_filters);
	if (mem != BTLBF_HOST && mem != BTLBF_DEVICE)
		return btlbf_set_error(BTLBF_EINVAL, "mem must be BTLBF_HOST or BTLBF_DEVICE");
	DeviceGuard g(device);
	if (!g.ok)
		return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	InBuf h, v, pb;
	OutBuf pa, be, to; // updated: the caller's counts go in first
	int rc;
	if ((rc = h.prepare(hits, n_rows * n_filters * 4, mem, s)) || (rc = v.prepare(valid, n_rows * 4, mem, s)) ||
	    (rc = pb.prepare(pass_bits, n_rows * 4, mem, s)) || (rc = pa.prepare(passed, n_filters * 8, mem, false, s, true)) ||
	    (rc = be.prepare(best, n_filters * 8, mem, false, s, true)) || (rc = to.prepare(totals4, 4 * 8, mem, false, s, true)))
		return rc;
	HIP_TRY(launch_screen_tally(h.as<uint32_t>(), v.as<uint32_t>(), pb.as<uint32_t>(), n_rows, n_filters,
	                            pa.as<unsigned long long>(), be.as<unsigned long long>(), to.as<unsigned long long>(), nullptr,
	                            s));
	if (mem == BTLBF_DEVICE)
		return BTLBF_OK;
	if ((rc = pa.finish(s)) || (rc = be.finish(s)) || (rc = to.finish(s)))
		return rc;
	HIP_TRY(hipStreamSynchronize(s));
	return BTLBF_OK;
}

// -------------------------------------------------------------------------------------------------
// the file handle (a file and its parser thread: Side, fastx_side.hpp)
// -------------------------------------------------------------------------------------------------
struct btlbf_screen_file {
	ScreenSet set;
	int device = 0;
	btlbf_screen_params par{};
	Side side;
	HostBatch cur;
	hipStream_t copy_s = nullptr, comp_s = nullptr;
	// grow only, free themselves.  Device: two slots of a batch (bases, offsets, the three result arrays), the bitmaps,
	// the totals (passed[n], best[n], totals4, windows); pinned: the slots' offsets and result sets
	DevScratch d_bases[2], d_starts[2], d_hits[2], d_valid[2], d_pass[2], cols, d_tot;
	PinScratch h_starts[2], h_hits[2], h_valid[2], h_pass[2];
	int slot = 0;
	uint64_t next_row = 0;
	bool ended = false;
	int end_rc = BTLBF_OK; // what the call that reached the end returned, and every later call returns
	std::string end_err;
	uint64_t n_batches = 0, n_bases = 0;

	~btlbf_screen_file() // the buffers go after this: none while work is pending
	{
		side.stop();
		for (hipStream_t s : {comp_s, copy_s})
			if (s) {
				(void)hipStreamSynchronize(s);
				(void)hipStreamDestroy(s);
			}
	}
	template <class Buf>
	bool room(Buf& b, uint64_t n) { return b.keep_room(n ? n : 16, device); }
	unsigned long long* tot() const { return d_tot.as<unsigned long long>(); }
};

namespace {

int end_input(btlbf_screen_file* c, int rc)
{
	c->ended = true;
	c->end_rc = rc;
	c->end_err = rc ? btlbf_last_error() : "";
	return rc;
}

// the next parser batch through slot c->slot: *n_rows == 0 at the end of input
int next_rows(btlbf_screen_file* c, uint64_t* n_rows, bool want_rows)
{
	*n_rows = 0;
	HostBatch& b = c->cur;
	int rc = c->side.take(&b);
	if (rc)
		return end_input(c, rc);
	if (b.ns == 0)
		return end_input(c, BTLBF_OK);
	const int sl = c->slot;
	const unsigned nf = c->set.n;
	const uint64_t n = b.ns, b0 = b.starts[0], len = b.starts[n] - b0;
	if (!c->room(c->d_bases[sl], len + 64) || !c->room(c->d_starts[sl], (n + 1) * 8) || !c->room(c->h_starts[sl], (n + 1) * 8) ||
	    !c->room(c->d_hits[sl], n * nf * 4) || !c->room(c->d_valid[sl], n * 4) || !c->room(c->d_pass[sl], n * 4))
		return fail(BTLBF_ENOMEM, "screen file: a batch of %llu bytes and %llu rows", (unsigned long long)len,
		            (unsigned long long)n);
	uint64_t* hs = c->h_starts[sl].as<uint64_t>();
	for (uint64_t i = 0; i <= n; ++i)
		hs[i] = b.starts[i] - b0;
	if (len)
		HIP_TRY(hipMemcpyAsync(c->d_bases[sl].p, b.bases + b0, len, hipMemcpyHostToDevice, c->copy_s));
	HIP_TRY(hipMemcpyAsync(c->d_starts[sl].p, hs, (n + 1) * 8, hipMemcpyHostToDevice, c->copy_s));
	HIP_TRY(hipStreamSynchronize(c->copy_s)); // the batch is on the device before the compute stream reads it
	uint32_t *d_hits = c->d_hits[sl].as<uint32_t>(), *d_valid = c->d_valid[sl].as<uint32_t>(),
	         *d_pass = c->d_pass[sl].as<uint32_t>();
	{
		SetLock lk;
		lk.lock(c->set);
		const LayoutParams lay{c->d_starts[sl].as<uint64_t>(), n, 0};
		if ((rc = screen_device(c->set, c->d_bases[sl].as<uint8_t>(), len, lay, n, c->par, d_hits, d_valid, d_pass, c->cols,
		                        c->comp_s)))
			return rc;
		HIP_TRY(launch_screen_tally(d_hits, d_valid, d_pass, n, nf, c->tot(), c->tot() + nf, c->tot() + 2 * nf,
		                            c->tot() + 2 * nf + 4, c->comp_s));
		if (want_rows) {
			if (!c->room(c->h_hits[sl], n * nf * 4) || !c->room(c->h_valid[sl], n * 4) || !c->room(c->h_pass[sl], n * 4))
				return fail(BTLBF_ENOMEM, "screen file: pinned results of %llu rows", (unsigned long long)n);
			HIP_TRY(hipMemcpyAsync(c->h_hits[sl].p, d_hits, n * nf * 4, hipMemcpyDeviceToHost, c->comp_s));
			HIP_TRY(hipMemcpyAsync(c->h_valid[sl].p, d_valid, n * 4, hipMemcpyDeviceToHost, c->comp_s));
			HIP_TRY(hipMemcpyAsync(c->h_pass[sl].p, d_pass, n * 4, hipMemcpyDeviceToHost, c->comp_s));
		}
		HIP_TRY(hipStreamSynchronize(c->comp_s)); // the filters are read under their locks
	}
	++c->n_batches;
	c->n_bases += len;
	*n_rows = n;
	return BTLBF_OK;
}

} // namespace

extern "C" int btlbf_screen_fastx_open(btlbf_screen_file** out, btlbf_filter* const* filters, unsigned n_filters,
                                       const char* path, uint32_t flags, const btlbf_screen_params* p, uint64_t batch_bytes)
{
	if (!out || !path)
		return btlbf_set_error(BTLBF_EINVAL, "screen file: null argument");
	*out = nullptr;
	ScreenSet set;
	int rc = check_set(set, filters, n_filters, p);
	if (rc)
		return rc;
	if (FILE* fp = fopen(path, "rb"))
		fclose(fp);
	else
		return btlbf_set_error(BTLBF_EIO, "file \"%s\" could not be read.", path);
	unsigned k = 0;
	{
		SetLock lk;
		lk.lock(set);
		if ((rc = check_compatible(set)))
			return rc;
		k = set.f[0]->k;
	}
	btlbf_screen_file* c = new (std::nothrow) btlbf_screen_file;
	if (!c)
		return btlbf_set_error(BTLBF_ENOMEM, "screen file: out of memory");
	c->set = set;
	c->device = set.f[0]->device;
	c->par = *p;
	DeviceGuard g(c->device);
	if (!g.ok) {
		delete c;
		return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", set.f[0]->device);
	}
	const uint32_t pf = (flags & (BTLBF_FASTX_LINES | BTLBF_FASTX_PAGEABLE)) | BTLBF_FASTX_WHOLE;
	const uint64_t tot_bytes = (2 * (uint64_t)set.n + 5) * 8;
	hipError_t e = hipSuccess;
	// the parser's pinned buffers need the device to be current
	if ((rc = btlbf_fastx_open(&c->side.r, path, pf, k, batch_bytes ? batch_bytes : 64ull << 20)))
		goto bad;
	if (!c->d_tot.grow(tot_bytes, c->device))
		e = hipErrorOutOfMemory;
	if (e != hipSuccess || (e = hipStreamCreateWithFlags(&c->copy_s, hipStreamNonBlocking)) != hipSuccess ||
	    (e = hipStreamCreateWithFlags(&c->comp_s, hipStreamNonBlocking)) != hipSuccess ||
	    (e = hipMemset(c->d_tot.p, 0, tot_bytes)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
		rc = fail(BTLBF_EHIP, "screen file: %s", hipGetErrorString(e));
		goto bad;
	}
	c->side.th = std::thread([c] { c->side.run(); });
	*out = c;
	return BTLBF_OK;
bad:
	delete c;
	return rc;
}

extern "C" int btlbf_screen_fastx_next(btlbf_screen_file* c, uint64_t* first_row, uint64_t* n_rows, const uint32_t** hits,
                                       const uint32_t** valid, const uint32_t** pass_bits)
{
	if (!c || !first_row || !n_rows)
		return btlbf_set_error(BTLBF_EINVAL, "screen file: null argument");
	const bool want_rows = hits || valid || pass_bits;
	if (want_rows && (!hits || !valid || !pass_bits))
		return btlbf_set_error(BTLBF_EINVAL, "screen file: the three result pointers are given together or not at all");
	*first_row = c->next_row;
	*n_rows = 0;
	if (c->ended)
		return c->end_rc ? btlbf_set_error(c->end_rc, "%s", c->end_err.c_str()) : BTLBF_OK;
	DeviceGuard g(c->device);
	c->slot ^= 1;
	uint64_t n = 0;
	const int rc = next_rows(c, &n, want_rows);
	if (rc) { // whatever failed, the batch is gone: the error is the answer from here on (rows must stay contiguous)
		if (!c->ended)
			end_input(c, rc);
		return rc;
	}
	*n_rows = n;
	c->next_row += n;
	if (want_rows) {
		*hits = n ? c->h_hits[c->slot].as<uint32_t>() : nullptr;
		*valid = n ? c->h_valid[c->slot].as<uint32_t>() : nullptr;
		*pass_bits = n ? c->h_pass[c->slot].as<uint32_t>() : nullptr;
	}
	return BTLBF_OK;
}

extern "C" int btlbf_screen_fastx_tally(btlbf_screen_file* c, uint64_t* passed, uint64_t* best, uint64_t* totals4)
{
	if (!c || !passed || !best || !totals4)
		return btlbf_set_error(BTLBF_EINVAL, "screen file: null argument");
	DeviceGuard g(c->device);
	const unsigned nf = c->set.n;
	HIP_TRY(hipStreamSynchronize(c->comp_s));
	HIP_TRY(hipMemcpy(passed, c->tot(), nf * 8, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(best, c->tot() + nf, nf * 8, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(totals4, c->tot() + 2 * nf, 4 * 8, hipMemcpyDeviceToHost));
	return BTLBF_OK;
}

extern "C" void btlbf_screen_fastx_close(btlbf_screen_file* c)
{
	if (!c)
		return;
	DeviceGuard g(c->device);
	delete c;
}

extern "C" int btlbf_screen_fastx(btlbf_filter* const* filters, unsigned n_filters, const char* path, uint32_t flags,
                                  const btlbf_screen_params* p, uint64_t batch_bytes, uint64_t* passed, uint64_t* best,
                                  uint64_t* totals4, btlbf_fastx_stats* stats)
{
	if (!passed || !best || !totals4)
		return btlbf_set_error(BTLBF_EINVAL, "screen file: null argument");
	const double t0 = now_s();
	btlbf_screen_file* c = nullptr;
	int rc = btlbf_screen_fastx_open(&c, filters, n_filters, path, flags, p, batch_bytes);
	if (rc)
		return rc;
	uint64_t first = 0, n = 0;
	do
		rc = btlbf_screen_fastx_next(c, &first, &n, nullptr, nullptr, nullptr);
	while (rc == BTLBF_OK && n);
	if (rc == BTLBF_OK)
		rc = btlbf_screen_fastx_tally(c, passed, best, totals4);
	if (stats) {
		memset(stats, 0, sizeof *stats);
		stats->n_batches = c->n_batches;
		stats->n_bases = c->n_bases;
		unsigned long long win = 0;
		DeviceGuard g(c->device);
		if (hipMemcpy(&win, c->tot() + 2 * c->set.n + 4, 8, hipMemcpyDeviceToHost) == hipSuccess)
			stats->n_windows = win;
		std::lock_guard<std::mutex> lk(c->side.mu);
		stats->n_records = btlbf_fastx_records(c->side.r);
		stats->seconds_parse = c->side.seconds_parse;
	}
	std::string err = rc ? btlbf_last_error() : "";
	btlbf_screen_fastx_close(c);
	if (stats)
		stats->seconds_total = now_s() - t0;
	return rc ? btlbf_set_error(rc, "%s", err.c_str()) : BTLBF_OK;
}
