// csrc/capi.cpp -- the core of the C ABI declared in include/btlbf.h (host side; compiled by hipcc).
//
// Errors, the lazy-clear protocol, the staging pool and the mailboxes, the hash / modulo / spaced-seed parameter
// blocks, the filter object with its lifetime, modes, profiling and accessors, clear / upload / download.  The
// other host units (host_internal.hpp lists what they share): host_io.cpp (BTLBloomFilter_v1 files), host_seq.cpp (the
// sequence, hash-row and k-mer entry points), host_partition.cpp (the partitioned pipeline and the multi-GPU routing),
// host_aux.cpp (statistics, rank structure, position exchange, support), host_mibf.cpp (multi-index Bloom filter),
// fastx.cpp (FASTA/FASTQ reader).  There is deliberately no CPU implementation of any compute entry point in them.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

using namespace btlbf;

// -------------------------------------------------------------------------------------------------
// errors
// -------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

namespace btlbf {
// Every error return of this file passes here BEFORE the locals of the failing call are destroyed.  An error that
// comes after kernels were queued would otherwise hand pooled staging buffers (DevBuf) back to the pool -- and to
// the next call -- with that work still pending; so the device is drained first (errors are not a hot path).
int fail(int code, const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	if (hipDeviceSynchronize() != hipSuccess)
		(void)hipGetLastError();
	return code;
}
} // namespace btlbf

int btlbf_set_error(int code, const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	return code;
}

extern "C" const char* btlbf_last_error(void) { return g_err; }

extern "C" int btlbf_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

namespace {

uint64_t srol_n(uint64_t x, unsigned s)
{
	uint64_t lo = x & 0x1FFFFFFFFULL, hi = x >> 33;
	const unsigned a = s % 33, b = s % 31;
	if (a)
		lo = ((lo << a) | (lo >> (33 - a))) & 0x1FFFFFFFFULL;
	if (b)
		hi = ((hi << b) | (hi >> (31 - b))) & 0x7FFFFFFFULL;
	return (hi << 33) | lo;
}

const uint64_t kSeeds[4] = {kSeedA, kSeedC, kSeedG, kSeedT};
// forward / reverse-strand seed of a device base code (internal.hpp: codes 4..7 are raw bytes whose
// "complement" under c & cpOff is the byte itself)
uint64_t fwd_seed(unsigned c) { return kSeeds[c & 3]; }
uint64_t rev_seed(unsigned c) { return c < 4 ? kSeeds[c ^ 3] : kSeeds[c & 3]; }

uint64_t cbf_round_bytes(uint64_t b) // CountingBloomFilter.hpp:40-49
{
	const uint64_t r = b % 8;
	return r ? b + 8 - r : b;
}

} // namespace

namespace btlbf {

// stream s is about to carry out a pending clear: it first waits for the point of the clear on the caller's stream
hipError_t order_after_clear(btlbf_filter* f, hipStream_t s)
{
	if (!f->clear_ev_pending)
		return hipSuccess;
	f->clear_ev_pending = false;
	return hipStreamWaitEvent(s, f->clear_ev, 0);
}

// a pending btlbf_clear takes effect now, on the stream of the operation that needs the array
hipError_t materialize_clear(btlbf_filter* f, hipStream_t s)
{
	if (!f)
		return hipSuccess;
	if (!f->lazy_zero) {
		// an earlier call zeroed the array on ITS stream: a different stream waits for that zeroing (a per-thread
		// stream handle names a different stream in every host thread, so it always waits; waiting for an event of
		// one's own stream costs nothing)
		if (!f->zero_ev_pending)
			return hipSuccess;
		if (s == f->zero_stream && s != hipStreamPerThread)
			return hipSuccess;
		if (hipEventQuery(f->zero_ev) == hipSuccess) {
			f->zero_ev_pending = false;
			return hipSuccess;
		}
		(void)hipGetLastError(); // hipErrorNotReady is not an error
		return hipStreamWaitEvent(s, f->zero_ev, 0);
	}
	hipError_t e = order_after_clear(f, s);
	if (e != hipSuccess)
		return e;
	f->lazy_zero = false;
	e = hipMemsetAsync(f->d_data, 0, f->alloc_bytes, s);
	if (e != hipSuccess)
		return e;
	if (!f->zero_ev && (e = hipEventCreateWithFlags(&f->zero_ev, hipEventDisableTiming)) != hipSuccess)
		return e;
	if ((e = hipEventRecord(f->zero_ev, s)) != hipSuccess)
		return e;
	f->zero_stream = s;
	f->zero_ev_pending = true;
	return hipSuccess;
}

DevPool& dev_pool()
{
	static DevPool* pool = new DevPool(); // never destroyed: the HIP runtime may be gone by static destruction time
	return *pool;
}

// one per host thread AND device: the mapping is made under the device that is current (the filter's: every caller
// holds a DeviceGuard) and used for filters on that device only
Mailbox& mailbox()
{
	static thread_local std::map<int, Mailbox> boxes;
	int cur = 0;
	if (hipGetDevice(&cur) != hipSuccess)
		cur = 0;
	return boxes[cur];
}

void fill_hash_params(HashParams& hp, unsigned k, unsigned h)
{
	memset(&hp, 0, sizeof hp);
	hp.k = k;
	hp.h = h;
	hp.kms = (uint64_t)k * kMultiSeed;
	hp.use_pos_tab = k <= 128; // 128*k bytes of LDS; launchers may clear it when LDS is tight
	for (unsigned c = 0; c < kNumCodes; ++c) {
		const uint64_t s = fwd_seed(c), rc = rev_seed(c);
		hp.init_tab[c][0] = s;
		hp.init_tab[c][1] = srol_n(rc, k - 1);
		hp.in_tab[c][0] = s;
		hp.in_tab[c][1] = srol_n(rc, k);
		hp.out_tab[c][0] = srol_n(s, k);
		hp.out_tab[c][1] = rc;
	}
}

// The spaced-seed lists of a configuration, on the host alone: the checks of what the library accepts, the per-seed
// don't-care lists (dc), the union list (dcu) and the counts in hp that size the kernels' LDS tables.  No device call.
static int plan_spaced(HashParams& hp, const char* const* seeds, unsigned n_seeds, unsigned h2, std::vector<uint16_t>& dc,
                       std::vector<uint32_t>& dcu)
{
	const unsigned k = hp.k;
	if (n_seeds == 0 || n_seeds > (unsigned)kMaxSeeds || h2 == 0)
		return fail(BTLBF_EINVAL, "spaced seeds: need 1..%d seeds and h2 >= 1", kMaxSeeds);
	if ((uint64_t)n_seeds * h2 > (uint64_t)kMaxHash)
		return fail(BTLBF_EINVAL, "spaced seeds: n_seeds*h2 = %u exceeds %d", n_seeds * h2, kMaxHash);
	if (k > 1024)
		return fail(BTLBF_EINVAL, "spaced seeds: k = %u > 1024 unsupported", k);
	for (unsigned j = 0; j < n_seeds; ++j) {
		if (!seeds[j] || strlen(seeds[j]) != k)
			return fail(BTLBF_EINVAL, "spaced seed %u must have exactly k = %u characters", j, k);
		hp.dc_off[j] = (uint32_t)dc.size();
		for (unsigned i = 0; i < k; ++i)
			if (seeds[j][i] != '1') // parseSeed keeps the indices of non-'1' (stHashIterator.hpp:27-29)
				dc.push_back((uint16_t)i);
	}
	hp.dc_off[n_seeds] = (uint32_t)dc.size();
	// the union list (internal.hpp HashParams::dcu): distinct offsets with their seed masks, those of every seed first
	{
		std::map<unsigned, uint32_t> mask_of;
		for (unsigned j = 0; j < n_seeds; ++j)
			for (uint32_t d = hp.dc_off[j]; d < hp.dc_off[j + 1]; ++d)
				mask_of[dc[d]] |= 1u << j;
		const uint32_t all = n_seeds >= 32 ? 0xffffffffu : (1u << n_seeds) - 1;
		for (const auto& kv : mask_of)
			if (kv.second == all)
				dcu.push_back(kv.first | (kv.second << 16));
		hp.n_dcu_all = (uint32_t)dcu.size();
		// the others grouped by their mask, every group an even number of entries: the hash stage takes them in pairs
		// with one mask (seq_core.hpp); the filler is the "offset" k, the zero row behind the positional table
		std::map<uint32_t, std::vector<unsigned>> by_mask;
		for (const auto& kv : mask_of)
			if (kv.second != all)
				by_mask[kv.second].push_back(kv.first);
		for (const auto& g : by_mask) {
			for (unsigned off : g.second)
				dcu.push_back(off | (g.first << 16));
			if (g.second.size() % 2)
				dcu.push_back(k | (g.first << 16));
		}
		if (dcu.size() > kMaxDcu) {
			dcu.clear();
			hp.n_dcu_all = 0;
		}
		// two-base rows for the pairs (seq_core.hpp): the hash stage takes two pairs per trip, so an even number of
		// them -- a pair of fillers with an empty mask if need be; at most 16 rows (4 KB of LDS)
		hp.want_pair_rows = hp.n_pair_rows = 0;
		if (!dcu.empty()) {
			size_t pairs = (dcu.size() - hp.n_dcu_all) / 2;
			if (pairs % 2 && dcu.size() + 2 <= kMaxDcu) {
				dcu.push_back(k);
				dcu.push_back(k);
				++pairs;
			}
			if (pairs && pairs % 2 == 0 && pairs <= 16)
				hp.want_pair_rows = (uint32_t)pairs;
		}
		hp.n_dcu = (uint32_t)dcu.size();
	}
	hp.n_seeds = n_seeds;
	hp.h2 = h2;
	hp.h = n_seeds * h2;
	hp.use_pos_tab = 1; // spaced seeds are masked through the positional table (k <= 1024 checked above)
	// The positional table and the lists must fit the LDS of the direct kernels next to the tile image (internal.hpp
	// seq_lds_fits): decided here by arithmetic, so that a configuration is refused when it is set and no launcher ever
	// asks the runtime for more LDS than a workgroup has.
	if (!seq_lds_fits(hp))
		return fail(BTLBF_EINVAL,
		            "spaced seeds: k = %u with %u seeds (%u don't-care positions in all) needs %u bytes of LDS per workgroup, "
		            "%u are available",
		            k, n_seeds, (unsigned)dc.size(), seq_lds_dyn(hp) + kSeqStaticLds, kLdsPerWorkgroup);
	return BTLBF_OK;
}

// spaced-seed tables on the device; on success the caller owns *d_pos / *d_dc
int build_spaced(HashParams& hp, const char* const* seeds, unsigned n_seeds, unsigned h2,
                 uint64_t** d_pos, uint16_t** d_dc)
{
	std::vector<uint16_t> dc;
	std::vector<uint32_t> dcu;
	*d_pos = nullptr;
	{
		HashParams planned = hp;
		if (int rc = plan_spaced(planned, seeds, n_seeds, h2, dc, dcu))
			return rc;
		hp = planned;
	}
	const size_t dc_bytes = (dc.size() * 2 + 15) / 16 * 16;
	HIP_TRY(hipMalloc((void**)d_dc, dc_bytes + dcu.size() * 4 + 16));
	if (!dc.empty())
		HIP_TRY(hipMemcpy(*d_dc, dc.data(), dc.size() * 2, hipMemcpyHostToDevice));
	if (!dcu.empty())
		HIP_TRY(hipMemcpy(reinterpret_cast<uint8_t*>(*d_dc) + dc_bytes, dcu.data(), dcu.size() * 4, hipMemcpyHostToDevice));
	hp.dc_idx = *d_dc;
	hp.dcu = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(*d_dc) + dc_bytes);
	return BTLBF_OK;
}

void fill_mod(ModParams& m, uint64_t size, uint64_t lo, uint64_t len)
{
	memset(&m, 0, sizeof m);
	m.size = size;
	m.pow2 = (size & (size - 1)) == 0;
	m.mask = size - 1;
	// floor(2^64 / size) for size >= 2 that is not a power of two == floor((2^64-1)/size)
	m.magic = m.pow2 ? 0 : (~0ULL) / size;
	m.magic32 = (m.magic >> 32) || (size >> 63) ? 0 : (uint32_t)m.magic;
	m.neg_size = 0 - size;
	m.shard_lo = lo;
	m.shard_len = len;
	m.shard_shift = 0xffffffffu;
	if (len && (len & (len - 1)) == 0) {
		unsigned s = 0;
		while ((1ULL << s) < len)
			++s;
		m.shard_shift = s;
	}
}

int make_filter(btlbf_filter** out, int kind, uint64_t size, uint64_t size_bytes, unsigned shard_index,
                unsigned shard_count, unsigned h, unsigned k, unsigned thr, int device)
{
	if (!out)
		return fail(BTLBF_EINVAL, "null out pointer");
	*out = nullptr;
	const int cb = kind_counter_bytes(kind);
	if (cb < 0)
		return fail(BTLBF_EINVAL, "unknown filter kind %d", kind);
	if (cb > 1 && shard_count != 1)
		return refuse_wide("a shard of a wide counting filter");
	if (h == 0)
		return fail(BTLBF_EINVAL, "hash_num must be >= 1");
	if (k == 0 || k > 32768)
		return fail(BTLBF_EINVAL, "kmer_size must be in 1..32768");
	if (cb > 1 ? size < 1 : size < 8) // (8 bytes of wide counters are 4, 2 or 1 of them)
		return fail(BTLBF_EINVAL, "filter size %llu too small", (unsigned long long)size);
	if (shard_count == 0 || shard_index >= shard_count || size % shard_count ||
	    (shard_count > 1 && (size / shard_count) % 64))
		return fail(BTLBF_EINVAL, "shard %u of %u does not split %llu positions into multiples of 64",
		            shard_index, shard_count, (unsigned long long)size);
	if (btlbf_device_count() <= device || device < 0)
		return fail(BTLBF_EHIP, "no GPU %d (visible devices: %d): this library has no CPU path", device,
		            btlbf_device_count());
	DeviceGuard g(device);
	if (!g.ok)
		return fail(BTLBF_EHIP, "cannot select GPU %d", device);
	btlbf_filter* f = new btlbf_filter();
	f->kind = kind;
	f->device = device;
	f->size = size;
	f->size_bytes = size_bytes;
	f->h = h;
	f->k = k;
	f->thr = thr;
	f->shard_index = shard_index;
	f->shard_count = shard_count;
	const uint64_t len = size / shard_count;
	f->local_bytes = kind == BTLBF_BLOOM ? len / 8 : len;
	if (shard_count == 1)
		f->local_bytes = size_bytes;
	f->alloc_bytes = (f->local_bytes + 15) / 16 * 16;
	fill_mod(f->mod, size, (uint64_t)shard_index * len, len);
	fill_hash_params(f->hp, k, h);
	// (a wide counting filter has the direct path only: "partitioned" in the environment is not for it)
	if (const char* m = getenv("BTLBF_INSERT_MODE")) {
		if (!strcmp(m, "direct"))
			f->insert_mode = BTLBF_INSERT_DIRECT;
		else if (!strcmp(m, "partitioned") && cb <= 1)
			f->insert_mode = BTLBF_INSERT_PARTITIONED;
	}
	if (const char* m = getenv("BTLBF_QUERY_MODE")) {
		if (!strcmp(m, "direct"))
			f->query_mode = BTLBF_INSERT_DIRECT;
		else if (!strcmp(m, "partitioned") && cb <= 1)
			f->query_mode = BTLBF_INSERT_PARTITIONED;
	}
	hipError_t e = hipMalloc(&f->d_data, f->alloc_bytes);
	if (e != hipSuccess) {
		delete f;
		return fail(e == hipErrorOutOfMemory ? BTLBF_ENOMEM : BTLBF_EHIP, "hipMalloc(%llu bytes): %s",
		            (unsigned long long)f->alloc_bytes, hipGetErrorString(e));
	}
	f->lazy_zero = true; // a new filter is a cleared filter: zeroed by whoever touches the array first
	e = hipMalloc((void**)&f->d_scalar, 64);
	if (e == hipSuccess)
		e = hipDeviceSynchronize();
	if (e != hipSuccess) {
		(void)hipFree(f->d_data);
		delete f;
		return fail(BTLBF_EHIP, "filter initialisation: %s", hipGetErrorString(e));
	}
	*out = f;
	return BTLBF_OK;
}

int check_layout(const btlbf_layout* l, uint64_t len)
{
	if (!l)
		return BTLBF_OK;
	if (l->starts == nullptr && l->read_len && len % l->read_len)
		return fail(BTLBF_EINVAL, "len %llu is not a multiple of read_len %u", (unsigned long long)len,
		            l->read_len);
	return BTLBF_OK;
}

int make_view(SeqView& v, const char* seq, uint64_t len, const btlbf_layout* l, int mem, hipStream_t s)
{
	if (len && !seq)
		return fail(BTLBF_EINVAL, "null sequence buffer");
	int rc = check_layout(l, len);
	if (rc)
		return rc;
	if (l) {
		v.lay.n_seqs = l->n_seqs;
		v.lay.read_len = l->starts ? 0 : l->read_len;
	}
	if (mem == BTLBF_DEVICE) {
		v.d_seq = reinterpret_cast<const uint8_t*>(seq);
		if (l && l->starts)
			v.lay.starts = l->starts;
		return BTLBF_OK;
	}
	if (mem != BTLBF_HOST)
		return fail(BTLBF_EINVAL, "mem must be BTLBF_HOST or BTLBF_DEVICE");
	HIP_TRY(v.seq_buf.alloc_pooled(len + 16));
	if (len)
		HIP_TRY(hipMemcpyAsync(v.seq_buf.p, seq, len, hipMemcpyHostToDevice, s));
	v.d_seq = v.seq_buf.as<uint8_t>();
	if (l && l->starts) {
		if (l->starts[0] != 0 || l->starts[l->n_seqs] != len)
			return fail(BTLBF_EINVAL, "starts[0] must be 0 and starts[n_seqs] must equal len");
		HIP_TRY(v.starts_buf.alloc_pooled((l->n_seqs + 1) * 8));
		HIP_TRY(hipMemcpyAsync(v.starts_buf.p, l->starts, (l->n_seqs + 1) * 8, hipMemcpyHostToDevice, s));
		v.lay.starts = v.starts_buf.as<uint64_t>();
	}
	return BTLBF_OK;
}

SeqArgs base_args(const btlbf_filter* f, const SeqView& v, uint64_t len)
{
	SeqArgs a;
	memset(&a, 0, sizeof a);
	a.seq = v.d_seq;
	a.len = len;
	a.layout = v.lay;
	a.filter = f->d_data;
	a.mod = f->mod;
	a.hp = f->hp;
	a.threshold = f->thr;
	return a;
}

} // namespace btlbf

// -------------------------------------------------------------------------------------------------
// lifetime
// -------------------------------------------------------------------------------------------------
extern "C" int btlbf_create(btlbf_filter** out, int kind, uint64_t size, unsigned hash_num,
                            unsigned kmer_size, unsigned threshold, int device)
{
	if (kind == BTLBF_BLOOM) {
		if (size % 8 != 0) // BloomFilter.hpp:391-394
			return fail(BTLBF_EINVAL, "ERROR: Filter Size \"%llu\" is not a multiple of 8.",
			            (unsigned long long)size);
		return make_filter(out, kind, size, size / 8, 0, 1, hash_num, kmer_size, 0, device);
	}
	const uint64_t bytes = cbf_round_bytes(size);
	if (kind_counter_bytes(kind) > 1) // m_size = m_sizeInBytes / sizeof(T) counters (CountingBloomFilter.hpp:40-49)
		return make_filter(out, kind, bytes / (uint64_t)kind_counter_bytes(kind), bytes, 0, 1, hash_num, kmer_size,
		                   threshold, device);
	return make_filter(out, kind, bytes, bytes, 0, 1, hash_num, kmer_size, threshold, device);
}

extern "C" int btlbf_create_shard(btlbf_filter** out, int kind, uint64_t global_size,
                                  unsigned shard_index, unsigned shard_count, unsigned hash_num,
                                  unsigned kmer_size, unsigned threshold, int device)
{
	if (kind == BTLBF_BLOOM) {
		if (global_size % 8 != 0)
			return fail(BTLBF_EINVAL, "ERROR: Filter Size \"%llu\" is not a multiple of 8.",
			            (unsigned long long)global_size);
		return make_filter(out, kind, global_size, global_size / 8, shard_index, shard_count, hash_num,
		                   kmer_size, 0, device);
	}
	if (kind_counter_bytes(kind) > 1) {
		if (out)
			*out = nullptr;
		return refuse_wide("btlbf_create_shard");
	}
	const uint64_t bytes = cbf_round_bytes(global_size);
	return make_filter(out, kind, bytes, bytes, shard_index, shard_count, hash_num, kmer_size, threshold,
	                   device);
}

extern "C" int btlbf_destroy(btlbf_filter* f)
{
	if (!f)
		return BTLBF_OK;
	DeviceGuard g(f->device);
	if (f->clear_ev)
		(void)hipEventDestroy(f->clear_ev);
	if (f->zero_ev)
		(void)hipEventDestroy(f->zero_ev);
	if (f->screen_ev)
		(void)hipEventDestroy(f->screen_ev);
	(void)hipFree(f->d_data);
	(void)hipFree(f->d_scalar);
	(void)hipFree(f->d_pos_tab);
	(void)hipFree(f->d_dc_idx);
	f->part.release();
	f->split.release();
	f->flags.release();
	f->screen.release();
	delete f;
	return BTLBF_OK;
}

extern "C" int btlbf_set_insert_mode(btlbf_filter* f, int mode, uint64_t scratch_bytes)
{
	FilterLock lk__(f);
	if (!f || mode < BTLBF_INSERT_AUTO || mode > BTLBF_INSERT_PARTITIONED)
		return fail(BTLBF_EINVAL, "bad insert mode");
	if (is_wide(f) && mode == BTLBF_INSERT_PARTITIONED)
		return refuse_wide("btlbf_set_insert_mode(PARTITIONED)");
	f->insert_mode = mode;
	f->part_budget = scratch_bytes;
	return BTLBF_OK;
}

extern "C" int btlbf_release_scratch(btlbf_filter* f)
{
	FilterLock lk__(f);
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	DeviceGuard g(f->device);
	f->part.release();
	f->split.release();
	f->flags.release();
	f->screen.release();
	dev_pool().drain(f->device); // parked staging buffers of HOST-mode calls (every user has synchronised)
	return BTLBF_OK;
}

extern "C" int btlbf_set_profiling(btlbf_filter* f, int on)
{
	FilterLock lk__(f);
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	f->profiling = on != 0;
	return BTLBF_OK;
}

extern "C" int btlbf_get_profile(btlbf_filter* f, double* ms, unsigned* calls, int reset)
{
	FilterLock lk__(f);
	if (!f || !ms || !calls)
		return fail(BTLBF_EINVAL, "null argument");
	DeviceGuard g(f->device);
	for (auto& sp : f->spans) {
		float t = 0;
		if (hipEventSynchronize(sp.e1) == hipSuccess && hipEventElapsedTime(&t, sp.e0, sp.e1) == hipSuccess) {
			f->prof_ms[sp.slot] += t;
			f->prof_calls[sp.slot] += 1;
		}
		(void)hipEventDestroy(sp.e0);
		(void)hipEventDestroy(sp.e1);
	}
	f->spans.clear();
	for (int i = 0; i < BTLBF_PROF_SLOTS; ++i) {
		ms[i] = f->prof_ms[i];
		calls[i] = f->prof_calls[i];
		if (reset) {
			f->prof_ms[i] = 0;
			f->prof_calls[i] = 0;
		}
	}
	return BTLBF_OK;
}

extern "C" int btlbf_set_query_mode(btlbf_filter* f, int mode)
{
	FilterLock lk__(f);
	if (!f || mode < BTLBF_INSERT_AUTO || mode > BTLBF_INSERT_PARTITIONED)
		return fail(BTLBF_EINVAL, "bad query mode");
	if (is_wide(f) && mode == BTLBF_INSERT_PARTITIONED)
		return refuse_wide("btlbf_set_query_mode(PARTITIONED)");
	f->query_mode = mode;
	return BTLBF_OK;
}

// planning only (no device needed): would these spaced seeds be accepted, and the LDS they take in the direct kernels
extern "C" int btlbf_plan_spaced_lds(unsigned kmer_size, const char* const* seeds, unsigned n_seeds, unsigned h2,
                                     uint32_t* out2)
{
	if (!seeds || !out2 || kmer_size == 0 || kmer_size > 32768)
		return fail(BTLBF_EINVAL, "btlbf_plan_spaced_lds: bad argument");
	HashParams hp;
	fill_hash_params(hp, kmer_size, n_seeds * h2);
	std::vector<uint16_t> dc;
	std::vector<uint32_t> dcu;
	out2[0] = 0;
	out2[1] = kLdsPerWorkgroup;
	if (int rc = plan_spaced(hp, seeds, n_seeds, h2, dc, dcu))
		return rc;
	out2[0] = seq_lds_dyn(hp) + kSeqStaticLds;
	return BTLBF_OK;
}

extern "C" int btlbf_set_spaced_seeds(btlbf_filter* f, const char* const* seeds, unsigned n_seeds,
                                      unsigned h2)
{
	FilterLock lk__(f);
	if (!f || !seeds)
		return fail(BTLBF_EINVAL, "null argument");
	if (n_seeds * h2 != f->h)
		return fail(BTLBF_EINVAL, "n_seeds*h2 = %u must equal the filter's hash_num %u", n_seeds * h2, f->h);
	DeviceGuard g(f->device);
	HashParams hp;
	fill_hash_params(hp, f->k, f->h);
	uint64_t* dp = nullptr;
	uint16_t* dd = nullptr;
	int rc = build_spaced(hp, seeds, n_seeds, h2, &dp, &dd);
	if (rc) {
		(void)hipFree(dp);
		(void)hipFree(dd);
		return rc;
	}
	(void)hipFree(f->d_pos_tab);
	(void)hipFree(f->d_dc_idx);
	f->d_pos_tab = dp;
	f->d_dc_idx = dd;
	f->hp = hp;
	f->seed_strs.assign(seeds, seeds + n_seeds);
	return BTLBF_OK;
}

// -------------------------------------------------------------------------------------------------
// attributes
// -------------------------------------------------------------------------------------------------
extern "C" int btlbf_kind(const btlbf_filter* f) { return f->kind; }
extern "C" unsigned btlbf_counter_bytes(const btlbf_filter* f) { return counter_bytes(f); }
extern "C" uint64_t btlbf_size(const btlbf_filter* f) { return f->size; }
extern "C" uint64_t btlbf_size_bytes(const btlbf_filter* f) { return f->size_bytes; }
extern "C" uint64_t btlbf_local_bytes(const btlbf_filter* f) { return f->local_bytes; }
extern "C" unsigned btlbf_hash_num(const btlbf_filter* f) { return f->h; }
extern "C" unsigned btlbf_kmer_size(const btlbf_filter* f) { return f->k; }
extern "C" unsigned btlbf_threshold(const btlbf_filter* f) { return f->thr; }
extern "C" uint64_t btlbf_get_n_entry(const btlbf_filter* f) { return f->n_entry; }
extern "C" uint64_t btlbf_get_t_entry(const btlbf_filter* f) { return f->t_entry; }
extern "C" void btlbf_set_n_entry(btlbf_filter* f, uint64_t v) { f->n_entry = v; }
extern "C" void btlbf_set_t_entry(btlbf_filter* f, uint64_t v) { f->t_entry = v; }
extern "C" void* btlbf_device_ptr(const btlbf_filter* f_)
{
	if (!f_)
		return nullptr;
	btlbf_filter* f = const_cast<btlbf_filter*>(f_);
	FilterLock lk__(f);
	if (f->lazy_zero) { // a caller that looks at the raw array must see a pending clear
		DeviceGuard g(f->device);
		(void)materialize_clear(f, nullptr);
		(void)hipDeviceSynchronize();
	}
	f->ptr_exposed = true; // from now on btlbf_clear zeroes eagerly, on its stream: the pointer may be kept
	return f->d_data;
}
extern "C" int btlbf_device(const btlbf_filter* f) { return f->device; }

extern "C" int btlbf_clear(btlbf_filter* f, void* stream)
{
	FilterLock lk__(f);
	if (!f)
		return fail(BTLBF_EINVAL, "null filter");
	DeviceGuard g(f->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (f->ptr_exposed) { // someone may hold the raw pointer: zero now, in stream order
		f->lazy_zero = false;
		f->clear_ev_pending = false;
		HIP_TRY(hipMemsetAsync(f->d_data, 0, f->alloc_bytes, s));
		if (!f->zero_ev)
			HIP_TRY(hipEventCreateWithFlags(&f->zero_ev, hipEventDisableTiming));
		HIP_TRY(hipEventRecord(f->zero_ev, s));
		f->zero_stream = s;
		f->zero_ev_pending = true;
		return BTLBF_OK;
	}
	// lazy: zeroed by whoever touches the array next (see btlbf_filter::lazy_zero), after this point of `stream`
	if (!f->clear_ev)
		HIP_TRY(hipEventCreateWithFlags(&f->clear_ev, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(f->clear_ev, s));
	f->clear_ev_pending = true;
	f->lazy_zero = true;
	return BTLBF_OK;
}

extern "C" int btlbf_upload(btlbf_filter* f, const void* src, uint64_t offset, uint64_t nbytes)
{
	FilterLock lk__(f);
	if (!f || (!src && nbytes))
		return fail(BTLBF_EINVAL, "null argument");
	if (offset + nbytes > f->local_bytes)
		return fail(BTLBF_EINVAL, "upload range exceeds the filter");
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(static_cast<uint8_t*>(f->d_data) + offset, src, nbytes, hipMemcpyHostToDevice));
	return BTLBF_OK;
}

extern "C" int btlbf_download(const btlbf_filter* f, void* dst, uint64_t offset, uint64_t nbytes)
{
	FilterLock lk__(f);
	if (!f || (!dst && nbytes))
		return fail(BTLBF_EINVAL, "null argument");
	if (offset + nbytes > f->local_bytes)
		return fail(BTLBF_EINVAL, "download range exceeds the filter");
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize()); // DEVICE-mode calls may have run on non-blocking user streams
	HIP_TRY(hipMemcpy(dst, static_cast<const uint8_t*>(f->d_data) + offset, nbytes, hipMemcpyDeviceToHost));
	return BTLBF_OK;
}
