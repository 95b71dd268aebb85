// csrc/host_card.cpp -- the k-mer cardinality sketch: btlbf_card_* (contracts and the sketch's definition: include/btlbf.h;
// kernels: card_kernels.hip).
//
// A sketch owns its table, the bit per counter the fused kernel marks wrapped counters in, and the three totals, all on
// one device.  Every entry point checks its arguments before any HIP call, then takes the sketch's lock.  add_seqs is
// the one call that runs on the caller's stream; the others wait for the whole device first (a BTLBF_DEVICE add may
// still be queued on a stream the NULL stream does not wait for) and return finished.  The file call feeds add's core
// from the ordered reader of fastx_side.hpp through two device slots.  The solver is host arithmetic alone.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"
#include "fastx_side.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

using namespace btlbf;

namespace {

struct CardLock {
	const btlbf_card* c;
	explicit CardLock(const btlbf_card* c_) : c(c_) { c->mu.lock(); }
	~CardLock() { c->mu.unlock(); }
	CardLock(const CardLock&) = delete;
	CardLock& operator=(const CardLock&) = delete;
};

int check_shape(unsigned kmer_size, unsigned sample_bits, unsigned table_bits)
{
	if (kmer_size == 0 || kmer_size > 32768)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: kmer_size must be 1..32768, not %u", kmer_size);
	if (sample_bits > kCardMaxSampleBits)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: sample_bits must be 0..%u, not %u", kCardMaxSampleBits, sample_bits);
	if (table_bits < kCardMinTableBits || table_bits > kCardMaxTableBits)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: table_bits must be %u..%u, not %u", kCardMinTableBits,
		                       kCardMaxTableBits, table_bits);
	return BTLBF_OK;
}

int check_hist(unsigned n_hist)
{
	if (n_hist < kCardMinHist || n_hist > kCardMaxHist)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: n_hist must be %u..%u, not %u", kCardMinHist, kCardMaxHist, n_hist);
	return BTLBF_OK;
}

int no_gpu(int device) { return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", device); }

// the windows of d_seq[0, len) into the sketch, queued on s (the sketch is locked, its device current)
int add_device(btlbf_card* c, const uint8_t* d_seq, uint64_t len, const LayoutParams& lay, hipStream_t s)
{
	CardArgs a;
	memset(&a, 0, sizeof a);
	a.seq = d_seq;
	a.len = len;
	a.layout = lay;
	a.hp = c->hp;
	a.table = c->d_table;
	a.wrapped = c->d_wrapped;
	a.table_bits = c->table_bits;
	a.sample_bits = c->sample_bits;
	a.totals3 = c->d_tot;
	HIP_TRY(launch_card(a, s));
	return BTLBF_OK;
}

// t[0, n_hist) on the host; the device has been synchronised by the caller, who holds the lock
int histogram_locked(btlbf_card* c, uint64_t* t, unsigned n_hist)
{
	if (!c->hist.keep_room((uint64_t)n_hist * 8, c->device))
		return fail(BTLBF_ENOMEM, "cardinality: %u histogram words", n_hist);
	HIP_TRY(hipMemsetAsync(c->hist.p, 0, (uint64_t)n_hist * 8, nullptr));
	HIP_TRY(launch_card_hist(c->d_table, c->table_bits, n_hist, c->hist.as<unsigned long long>(), nullptr));
	HIP_TRY(hipMemcpy(t, c->hist.p, (uint64_t)n_hist * 8, hipMemcpyDeviceToHost));
	return BTLBF_OK;
}

// the solver on checked arguments: phi is scratch of n_hist doubles; returns EINVAL with nothing written
int solve_checked(const uint64_t* t, unsigned n_hist, unsigned sample_bits, unsigned table_bits, btlbf_card_estimate* est,
                  double* f)
{
	const uint64_t R64 = 1ull << table_bits;
	uint64_t sum = 0;
	for (unsigned i = 0; i < n_hist; ++i) {
		if (t[i] > R64 - sum)
			return btlbf_set_error(BTLBF_EINVAL, "cardinality: the histogram holds more than 2^%u counters", table_bits);
		sum += t[i];
	}
	if (sum != R64)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: the histogram holds %llu counters, the table 2^%u",
		                       (unsigned long long)sum, table_bits);
	if (t[0] == 0)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: the table is full (no empty counter): raise table_bits or "
		                                     "sample_bits");
	const double R = (double)R64;
	const double t0 = (double)t[0];
	const double L = (double)table_bits * log(2.0) - log(t0);
	const double F0 = t[0] == R64 ? 0.0 : ldexp(L, (int)(table_bits + sample_bits));
	std::vector<double> phi(n_hist, 0.0);
	f[0] = 0.0;
	for (unsigned i = 1; i + 1 < n_hist; ++i) {
		double v = 0.0;
		if (t[0] != R64) {
			double s = 0.0;
			for (unsigned j = 1; j < i; ++j)
				s += (double)j * (double)t[i - j] * phi[j];
			v = (double)t[i] / (t0 * L) - s / ((double)i * t0);
		}
		phi[i] = v;
		f[i] = fabs(v) * F0;
	}
	est->distinct = F0;
	est->singletons = f[1];
	est->occupancy = 1.0 - t0 / R;
	est->windows = est->clean_windows = est->sampled = 0;
	est->overflow_buckets = t[n_hist - 1];
	return BTLBF_OK;
}

} // namespace

extern "C" int btlbf_card_create(btlbf_card** out, unsigned kmer_size, unsigned sample_bits, unsigned table_bits, int device)
{
	if (!out)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: null argument");
	*out = nullptr;
	int rc = check_shape(kmer_size, sample_bits, table_bits);
	if (rc)
		return rc;
	if (device < 0 || btlbf_device_count() <= device)
		return btlbf_set_error(BTLBF_EHIP, "no GPU %d: this library has no CPU path", device);
	DeviceGuard g(device);
	if (!g.ok)
		return no_gpu(device);
	btlbf_card* c = new (std::nothrow) btlbf_card;
	if (!c)
		return btlbf_set_error(BTLBF_ENOMEM, "cardinality: out of memory");
	c->k = kmer_size;
	c->sample_bits = sample_bits;
	c->table_bits = table_bits;
	c->device = device;
	fill_hash_params(c->hp, kmer_size, 1);
	hipError_t e;
	if ((e = hipMalloc(reinterpret_cast<void**>(&c->d_table), c->table_bytes())) != hipSuccess ||
	    (e = hipMalloc(reinterpret_cast<void**>(&c->d_wrapped), c->wrapped_bytes())) != hipSuccess ||
	    (e = hipMalloc(reinterpret_cast<void**>(&c->d_tot), 3 * 8)) != hipSuccess ||
	    (e = hipMemset(c->d_table, 0, c->table_bytes())) != hipSuccess ||
	    (e = hipMemset(c->d_wrapped, 0, c->wrapped_bytes())) != hipSuccess || (e = hipMemset(c->d_tot, 0, 3 * 8)) != hipSuccess ||
	    (e = hipDeviceSynchronize()) != hipSuccess) {
		rc = fail(e == hipErrorOutOfMemory ? BTLBF_ENOMEM : BTLBF_EHIP, "cardinality: a table of 2^%u counters: %s", table_bits,
		          hipGetErrorString(e));
		btlbf_card_destroy(c);
		return rc;
	}
	*out = c;
	return BTLBF_OK;
}

extern "C" void btlbf_card_destroy(btlbf_card* c)
{
	if (!c)
		return;
	{
		DeviceGuard g(c->device);
		for (void* p : {static_cast<void*>(c->d_table), static_cast<void*>(c->d_wrapped), static_cast<void*>(c->d_tot)})
			if (p)
				(void)hipFree(p); // synchronises with work in flight
		c->hist.release();
	}
	delete c;
}

extern "C" int btlbf_card_clear(btlbf_card* c)
{
	if (!c)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: null argument");
	CardLock lk(c);
	DeviceGuard g(c->device);
	if (!g.ok)
		return no_gpu(c->device);
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemset(c->d_table, 0, c->table_bytes()));
	HIP_TRY(hipMemset(c->d_tot, 0, 3 * 8));
	HIP_TRY(hipDeviceSynchronize());
	return BTLBF_OK;
}

extern "C" int btlbf_card_add_seqs(btlbf_card* c, const char* seq, uint64_t len, const btlbf_layout* layout, int mem,
                                   void* stream)
{
	if (!c || (len && !seq))
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: null argument");
	if (mem != BTLBF_HOST && mem != BTLBF_DEVICE)
		return btlbf_set_error(BTLBF_EINVAL, "mem must be BTLBF_HOST or BTLBF_DEVICE");
	if (layout && !layout->starts && layout->read_len && len % layout->read_len)
		return btlbf_set_error(BTLBF_EINVAL, "len %llu is not a multiple of read_len %u", (unsigned long long)len,
		                       layout->read_len);
	if (layout && layout->starts && mem == BTLBF_HOST) {
		if (layout->starts[0] != 0 || layout->starts[layout->n_seqs] != len)
			return btlbf_set_error(BTLBF_EINVAL, "starts[0] must be 0 and starts[n_seqs] must equal len");
		for (uint64_t i = 0; i < layout->n_seqs; ++i)
			if (layout->starts[i + 1] < layout->starts[i])
				return btlbf_set_error(BTLBF_EINVAL, "starts must not decrease");
	}
	if (len == 0)
		return BTLBF_OK;
	CardLock lk(c);
	DeviceGuard g(c->device);
	if (!g.ok)
		return no_gpu(c->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	SeqView v;
	int rc = make_view(v, seq, len, layout, mem, s);
	if (rc)
		return rc;
	if ((rc = add_device(c, v.d_seq, len, v.lay, s)))
		return rc;
	if (mem == BTLBF_HOST)
		HIP_TRY(hipStreamSynchronize(s)); // the staging buffers go back to the pool on return
	return BTLBF_OK;
}

extern "C" int btlbf_card_add_fastx(btlbf_card* c, const char* path, uint32_t flags, uint64_t batch_bytes,
                                    btlbf_fastx_stats* stats)
{
	if (!c || !path)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: null argument");
	if (FILE* fp = fopen(path, "rb"))
		fclose(fp);
	else
		return btlbf_set_error(BTLBF_EIO, "file \"%s\" could not be read.", path);
	const double t0 = now_s();
	if (batch_bytes == 0) {
		batch_bytes = 64ull << 20;
		// tests: batches of a few KiB, so that small files take the slot rotation and the cuts that real inputs take
		if (const char* e = getenv("BTLBF_FASTX_DEV_BYTES"))
			if (const uint64_t v = strtoull(e, nullptr, 10))
				batch_bytes = v;
	}
	CardLock lk(c);
	DeviceGuard g(c->device);
	if (!g.ok)
		return no_gpu(c->device);
	// declared in the order they must go in reverse: the parser thread ends first, then the streams are drained and
	// destroyed, then the slots are freed
	struct Loop {
		DevScratch d_bases[2], d_starts[2];
		hipStream_t copy_s = nullptr, comp_s = nullptr;
		Side side;
		~Loop()
		{
			side.stop();
			for (hipStream_t s : {comp_s, copy_s})
				if (s) {
					(void)hipStreamSynchronize(s);
					(void)hipStreamDestroy(s);
				}
		}
	} lp;
	btlbf_fastx_stats st;
	memset(&st, 0, sizeof st);
	unsigned long long before[3] = {0, 0, 0}, after[3] = {0, 0, 0};
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(before, c->d_tot, sizeof before, hipMemcpyDeviceToHost));
	HIP_TRY(hipStreamCreateWithFlags(&lp.copy_s, hipStreamNonBlocking));
	HIP_TRY(hipStreamCreateWithFlags(&lp.comp_s, hipStreamNonBlocking));
	const uint32_t pf = flags & (BTLBF_FASTX_LINES | BTLBF_FASTX_PAGEABLE | BTLBF_FASTX_WHOLE);
	int rc = btlbf_fastx_open(&lp.side.r, path, pf, c->k, batch_bytes); // (pinned buffers: the device is current)
	if (rc)
		return rc;
	Side& side = lp.side;
	side.th = std::thread([&side] { side.run(); });
	// the copies of a batch into slot sl, queued on the copy stream
	auto stage = [&](const HostBatch& b, int sl) -> int {
		if (b.starts[0] != 0 || b.starts[b.ns] != b.nb)
			return fail(BTLBF_EINVAL, "internal error: a parser batch of %llu bytes with offsets %llu..%llu",
			            (unsigned long long)b.nb, (unsigned long long)b.starts[0], (unsigned long long)b.starts[b.ns]);
		if (!lp.d_bases[sl].keep_room(b.nb + 64, c->device) || !lp.d_starts[sl].keep_room((b.ns + 1) * 8, c->device))
			return fail(BTLBF_ENOMEM, "cardinality: a batch of %llu bytes", (unsigned long long)b.nb);
		if (b.nb)
			HIP_TRY(hipMemcpyAsync(lp.d_bases[sl].p, b.bases, b.nb, hipMemcpyHostToDevice, lp.copy_s));
		HIP_TRY(hipMemcpyAsync(lp.d_starts[sl].p, b.starts, (b.ns + 1) * 8, hipMemcpyHostToDevice, lp.copy_s));
		return BTLBF_OK;
	};
	HostBatch cur;
	int sl = 0;
	if ((rc = side.take(&cur)) || (cur.ns && (rc = stage(cur, sl))))
		return rc;
	while (cur.ns) {
		// batch `cur` is on the device before its host buffers go back to the parser, which take() does; the kernel of
		// the batch before it has finished with the other slot (synchronised below) before the next copy goes there
		HIP_TRY(hipStreamSynchronize(lp.copy_s));
		const LayoutParams lay{lp.d_starts[sl].as<uint64_t>(), cur.ns, 0};
		if ((rc = add_device(c, lp.d_bases[sl].as<uint8_t>(), cur.nb, lay, lp.comp_s)))
			return rc;
		++st.n_batches;
		st.n_bases += cur.nb;
		HostBatch nxt;
		if ((rc = side.take(&nxt)) || (nxt.ns && (rc = stage(nxt, sl ^ 1))))
			return rc;
		HIP_TRY(hipStreamSynchronize(lp.comp_s));
		cur = nxt;
		sl ^= 1;
	}
	HIP_TRY(hipMemcpy(after, c->d_tot, sizeof after, hipMemcpyDeviceToHost));
	{
		std::lock_guard<std::mutex> lk2(side.mu);
		st.seconds_parse = side.seconds_parse;
		st.n_records = btlbf_fastx_records(side.r); // the end of input has come: the parser thread is done
	}
	st.n_windows = after[1] - before[1];
	st.n_hits = after[2] - before[2];
	st.seconds_total = now_s() - t0;
	if (stats)
		*stats = st;
	return BTLBF_OK;
}

extern "C" int btlbf_card_merge(btlbf_card* dst, const btlbf_card* src)
{
	if (!dst || !src)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: null argument");
	if (dst == src)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality merge: a sketch cannot be merged into itself");
	// (two locks, in ascending address: two threads merging a into b and b into a cannot deadlock)
	const btlbf_card* first = dst < src ? dst : src;
	const btlbf_card* second = dst < src ? src : dst;
	CardLock l1(first), l2(second);
	if (dst->k != src->k || dst->sample_bits != src->sample_bits || dst->table_bits != src->table_bits ||
	    dst->device != src->device)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality merge: kmer_size %u, sample_bits %u, table_bits %u on device %d "
		                       "cannot take kmer_size %u, sample_bits %u, table_bits %u on device %d", dst->k, dst->sample_bits,
		                       dst->table_bits, dst->device, src->k, src->sample_bits, src->table_bits, src->device);
	DeviceGuard g(dst->device);
	if (!g.ok)
		return no_gpu(dst->device);
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(launch_card_merge(dst->d_table, src->d_table, dst->table_bits, dst->d_tot, src->d_tot, nullptr));
	HIP_TRY(hipDeviceSynchronize());
	return BTLBF_OK;
}

extern "C" int btlbf_card_download(btlbf_card* c, uint32_t* table, uint64_t* totals3)
{
	if (!c || !table || !totals3)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: null argument");
	CardLock lk(c);
	DeviceGuard g(c->device);
	if (!g.ok)
		return no_gpu(c->device);
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(table, c->d_table, c->table_bytes(), hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(totals3, c->d_tot, 3 * 8, hipMemcpyDeviceToHost));
	return BTLBF_OK;
}

extern "C" int btlbf_card_upload(btlbf_card* c, const uint32_t* table, const uint64_t* totals3)
{
	if (!c || !table || !totals3)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: null argument");
	CardLock lk(c);
	DeviceGuard g(c->device);
	if (!g.ok)
		return no_gpu(c->device);
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(c->d_table, table, c->table_bytes(), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(c->d_tot, totals3, 3 * 8, hipMemcpyHostToDevice));
	HIP_TRY(hipDeviceSynchronize());
	return BTLBF_OK;
}

extern "C" int btlbf_card_histogram(btlbf_card* c, uint64_t* t, unsigned n_hist)
{
	if (!c || !t)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: null argument");
	int rc = check_hist(n_hist);
	if (rc)
		return rc;
	CardLock lk(c);
	DeviceGuard g(c->device);
	if (!g.ok)
		return no_gpu(c->device);
	HIP_TRY(hipDeviceSynchronize());
	return histogram_locked(c, t, n_hist);
}

extern "C" int btlbf_card_solve(const uint64_t* t, unsigned n_hist, unsigned sample_bits, unsigned table_bits,
                                btlbf_card_estimate* est, double* f)
{
	if (!t || !est || !f)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: null argument");
	int rc = check_hist(n_hist);
	if (rc)
		return rc;
	if ((rc = check_shape(1, sample_bits, table_bits)))
		return rc;
	return solve_checked(t, n_hist, sample_bits, table_bits, est, f);
}

extern "C" int btlbf_card_estimate_now(btlbf_card* c, unsigned n_hist, btlbf_card_estimate* est, double* f)
{
	if (!c || !est || !f)
		return btlbf_set_error(BTLBF_EINVAL, "cardinality: null argument");
	int rc = check_hist(n_hist);
	if (rc)
		return rc;
	CardLock lk(c);
	DeviceGuard g(c->device);
	if (!g.ok)
		return no_gpu(c->device);
	HIP_TRY(hipDeviceSynchronize());
	std::vector<uint64_t> t(n_hist);
	unsigned long long tot[3];
	if ((rc = histogram_locked(c, t.data(), n_hist)))
		return rc;
	HIP_TRY(hipMemcpy(tot, c->d_tot, sizeof tot, hipMemcpyDeviceToHost));
	if ((rc = solve_checked(t.data(), n_hist, c->sample_bits, c->table_bits, est, f)))
		return rc;
	est->windows = tot[0];
	est->clean_windows = tot[1];
	est->sampled = tot[2];
	return BTLBF_OK;
}
