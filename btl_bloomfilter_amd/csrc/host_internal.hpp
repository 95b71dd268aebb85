// csrc/host_internal.hpp -- what the host units of the C ABI share, and only that: error plumbing, the filter object,
// its cached device scratch (DevScratch, PinScratch) and its lazy-clear protocol, the staging pool and the mailbox, parameter
// blocks, sequence views, and the entries of the sequence path into the partitioned pipeline.  Defined in: capi.cpp
// (errors, clear protocol, dev_pool, mailbox, parameter blocks, make_filter, views), host_seq.cpp (seq_precheck),
// host_partition.cpp (the pipeline; its planner's types are in host_partition.hpp, for host_query.cpp alone),
// host_query.cpp (contains_routed), host_aux.cpp (rank_build).  fastx.cpp uses btlbf_set_error alone.
#pragma once
#include "../../include/btlbf.h"
#include "internal.hpp"

#include <map>
#include <mutex>
#include <string>
#include <vector>

// set the thread-local message behind btlbf_last_error() and return `code` (capi.cpp)
int btlbf_set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

namespace btlbf {

// A device buffer its owner keeps between calls (DevScratch): hipMalloc / hipFree of tens of GB cost more than the
// kernels, so it only ever grows; release() (btlbf_release_scratch, btlbf_destroy) or the owner's end give it back.  Its
// pinned sibling (PinScratch) is what the host and a stream hand each other.  The caller has the device selected.
template <bool kPinned>
struct GrowOnly {
	void* p = nullptr;
	uint64_t bytes = 0;
	GrowOnly() = default;
	GrowOnly(const GrowOnly&) = delete;
	GrowOnly& operator=(const GrowOnly&) = delete;
	~GrowOnly() { release(); }
	// room for `need` bytes (the contents are not kept); false = there is none, and the buffer is then empty
	bool grow(uint64_t need, int device);
	// ... with a quarter to spare, so that a slightly larger batch of a file does not allocate again
	bool keep_room(uint64_t need, int device) { return need <= bytes || grow(need + need / 4, device); }
	void release()
	{
		if (p)
			(void)(kPinned ? hipHostFree(p) : hipFree(p)); // synchronises with work in flight
		p = nullptr;
		bytes = 0;
	}
	template <class T>
	T* as() const
	{
		return static_cast<T*>(p);
	}
};
using DevScratch = GrowOnly<false>;
using PinScratch = GrowOnly<true>;

} // namespace btlbf

// -------------------------------------------------------------------------------------------------
// filter object
// -------------------------------------------------------------------------------------------------
struct btlbf_filter {
	// every entry point that takes the filter holds this for its whole duration: a filter keeps device
	// scratch, event lists and a scalar buffer between calls, so concurrent callers are serialised here
	// (recursive: btlbf_store -> btlbf_store_shard)
	mutable std::recursive_mutex mu;
	int kind = BTLBF_BLOOM;
	int device = 0;
	uint64_t size = 0;        // global bits / counters
	uint64_t size_bytes = 0;  // global bytes
	uint64_t local_bytes = 0; // bytes held here
	uint64_t alloc_bytes = 0; // local_bytes rounded up to 16 (zero padded)
	unsigned h = 0, k = 0, thr = 0;
	double dfpr = 0.0;
	uint64_t n_entry = 0, t_entry = 0;
	unsigned bits_per_counter = 8;
	unsigned shard_index = 0, shard_count = 1;
	void* d_data = nullptr;
	// btlbf_clear is LAZY: it only sets this.  The next partitioned insert builds every segment from zero in LDS
	// and writes it (no memset of the array, no read sweep for that batch); any other entry point that touches
	// the array zeroes it first (materialize_clear)
	bool lazy_zero = false;
	// the clear is ordered on the caller's stream: clear_ev is recorded there, and whichever stream carries the
	// zeroing out (materialize_clear, or the fresh partitioned insert) waits for it first, so work that was queued
	// before the clear on the caller's stream cannot run after (or beside) the zeroing
	hipEvent_t clear_ev = nullptr;
	bool clear_ev_pending = false;
	// ... and the zeroing itself, once some stream carries it out, is an event too: a call on ANOTHER stream (another
	// host thread's BTLBF_STREAM_PER_THREAD, say) that finds lazy_zero already false must not look at the array
	// while that memset is still in flight -- it waits for zero_ev first (materialize_clear)
	hipEvent_t zero_ev = nullptr;
	hipStream_t zero_stream = nullptr;
	bool zero_ev_pending = false;
	// set once btlbf_device_ptr has handed the raw pointer out: the caller may keep it, so from then on a clear
	// zeroes eagerly on its stream (a lazily cleared array would show stale contents through that pointer)
	bool ptr_exposed = false;
	btlbf::ModParams mod{};
	btlbf::HashParams hp{};
	// spaced seeds
	uint64_t* d_pos_tab = nullptr;
	uint16_t* d_dc_idx = nullptr;
	std::vector<std::string> seed_strs; // as given to btlbf_set_spaced_seeds (a miBF made from this filter stores them)
	// small device scratch for counters
	unsigned long long* d_scalar = nullptr; // 4 x u64
	// partitioned insert (partition_kernels.hip): mode + cached scratch
	int insert_mode = BTLBF_INSERT_AUTO;
	int query_mode = BTLBF_INSERT_AUTO;
	btlbf::DevScratch part;
	btlbf::DevScratch split; // split query: compacted reads + their bitmaps
	btlbf::DevScratch flags; // split query: cold flags of the reads + their prefix sums (small)
	btlbf::DevScratch screen; // read screen (host_screen.cpp): the per-window bitmaps of a btlbf_screen_seqs call
	// ... which a BTLBF_DEVICE call leaves in use when it returns: screen_ev is recorded behind its last kernel, and the next
	// call that takes the scratch (under this filter's lock, on whatever stream) makes its stream wait for it first
	hipEvent_t screen_ev = nullptr;
	bool screen_ev_pending = false;
	uint64_t part_budget = 0; // 0 = derive from free HBM
	// optional per-kernel timing with HIP events on the launch stream (btlbf_set_profiling)
	bool profiling = false;
	struct Span {
		int slot;
		hipEvent_t e0, e1;
	};
	std::vector<Span> spans;
	double prof_ms[BTLBF_PROF_SLOTS] = {0};
	unsigned prof_calls[BTLBF_PROF_SLOTS] = {0};
};

// -------------------------------------------------------------------------------------------------
// k-mer cardinality sketch (host_card.cpp)
// -------------------------------------------------------------------------------------------------
struct btlbf_card {
	mutable std::recursive_mutex mu; // every entry point that takes the sketch holds it for its whole duration
	unsigned k = 0, sample_bits = 0, table_bits = 0;
	int device = 0;
	btlbf::HashParams hp{};              // plain ntHash, one value per window
	uint32_t* d_table = nullptr;         // 2^table_bits counters
	uint32_t* d_wrapped = nullptr;       // a bit per counter, all zero between launches (card_kernels.hip)
	unsigned long long* d_tot = nullptr; // totals3
	btlbf::DevScratch hist;              // the histogram call's n_hist words
	uint64_t counters() const { return 1ull << table_bits; }
	uint64_t table_bytes() const { return counters() * 4; }
	uint64_t wrapped_bytes() const { return counters() / 8; }
};

namespace btlbf {

// The kinds: a bit filter, or counters of 1, 2, 4 or 8 bytes (CountingBloomFilter<T>).  Bytes per counter of a kind:
// 0 for BTLBF_BLOOM, -1 for a kind there is none of.  The wide kinds (more than a byte) take the direct path only -- one
// fused launch per call on the whole filter (wide_counter_kernels.hip): no shards, no partitioned pipeline, no routing.
inline int kind_counter_bytes(int kind)
{
	switch (kind) {
	case BTLBF_BLOOM: return 0;
	case BTLBF_COUNTING8: return 1;
	case BTLBF_COUNTING16: return 2;
	case BTLBF_COUNTING32: return 4;
	case BTLBF_COUNTING64: return 8;
	default: return -1;
	}
}
inline unsigned counter_bytes(const btlbf_filter* f) { return (unsigned)kind_counter_bytes(f->kind); }
inline bool is_counting(const btlbf_filter* f) { return counter_bytes(f) != 0; }
inline bool is_wide(const btlbf_filter* f) { return counter_bytes(f) > 1; }
// what an entry point that a wide filter cannot take answers, before any HIP call: sets the message, returns EINVAL
inline int refuse_wide(const char* what)
{
	return btlbf_set_error(BTLBF_EINVAL, "%s: counters wider than a byte take the direct path only (no shards, no "
	                                     "partitioned pipeline, no routing)", what);
}

// Every error return of the host units passes here BEFORE the locals of the failing call are destroyed: it sets the
// message, drains the device (capi.cpp says why) and returns `code`
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                              \
	do {                                                                                           \
		hipError_t e__ = (expr);                                                                   \
		if (e__ != hipSuccess)                                                                     \
			return fail(BTLBF_EHIP, "%s failed: %s", #expr, hipGetErrorString(e__));               \
	} while (0)

struct FilterLock {
	const btlbf_filter* f;
	explicit FilterLock(const btlbf_filter* f_)
	  : f(f_)
	{
		if (f)
			f->mu.lock();
	}
	~FilterLock()
	{
		if (f)
			f->mu.unlock();
	}
	// give the filter back early: a read-only call that has launched its kernel (on the caller's own stream, with
	// the caller's own buffers) only waits from here on, and other threads' calls may as well run meanwhile
	void release()
	{
		if (f)
			f->mu.unlock();
		f = nullptr;
	}
	FilterLock(const FilterLock&) = delete;
	FilterLock& operator=(const FilterLock&) = delete;
};

// the lazy clear (capi.cpp): stream s is about to carry out a pending clear / a pending clear takes effect now on s
hipError_t order_after_clear(btlbf_filter* f, hipStream_t s);
hipError_t materialize_clear(btlbf_filter* f, hipStream_t s);

// every launch of a kernel that reads or writes the array directly goes through this check: an entry point that
// forgot MATERIALIZE would otherwise read uninitialised HBM (the fresh partitioned insert is the one legitimate
// user of a lazily cleared array and does not come this way)
#define REQUIRE_MATERIALIZED(f)                                                                               \
	do {                                                                                                      \
		if ((f)->lazy_zero)                                                                                   \
			return fail(BTLBF_EINVAL, "internal error: %s line %d launches on a lazily cleared array", __func__, \
			            __LINE__);                                                                            \
	} while (0)
#define MATERIALIZE(f, s)                                                                              \
	do {                                                                                               \
		hipError_t em__ = materialize_clear(const_cast<btlbf_filter*>(f), static_cast<hipStream_t>(s)); \
		if (em__ != hipSuccess)                                                                        \
			return fail(BTLBF_EHIP, "clearing the filter failed: %s", hipGetErrorString(em__));         \
	} while (0)

// times one kernel launch with a pair of events when profiling is on
struct ProfSpan {
	btlbf_filter* f;
	hipStream_t s;
	int idx = -1;
	ProfSpan(btlbf_filter* f_, int slot, hipStream_t s_)
	  : f(f_)
	  , s(s_)
	{
		if (!f->profiling)
			return;
		btlbf_filter::Span sp{slot, nullptr, nullptr};
		if (hipEventCreate(&sp.e0) != hipSuccess || hipEventCreate(&sp.e1) != hipSuccess)
			return;
		(void)hipEventRecord(sp.e0, s);
		f->spans.push_back(sp);
		idx = (int)f->spans.size() - 1;
	}
	~ProfSpan()
	{
		if (idx >= 0)
			(void)hipEventRecord(f->spans[idx].e1, s);
	}
};

struct DeviceGuard {
	int prev = -1;
	bool ok = true;
	explicit DeviceGuard(int dev)
	{
		if (hipGetDevice(&prev) != hipSuccess) {
			ok = false;
			return;
		}
		if (prev != dev && hipSetDevice(dev) != hipSuccess)
			ok = false;
	}
	~DeviceGuard()
	{
		if (prev >= 0)
			(void)hipSetDevice(prev);
	}
};

// Small device buffers of HOST-mode calls (staged sequences, result buffers, hash rows) come from a pool:
// hipMalloc + hipFree per call cost more than the kernels of a per-read or per-k-mer call (the drop-in shims'
// ntHashIterator, contains(kmer), insertAndCheck make one such call each).  Power-of-two size classes up to
// 64 MiB, per device, at most 512 MiB parked.  A pooled buffer goes back only when the call that used it has
// synchronised its stream (every HOST-mode entry point does before it returns), so no work is pending on it.
struct DevPool {
	static constexpr size_t kMaxClass = 64u << 20, kMaxParked = 512u << 20;
	std::mutex mu;
	std::map<std::pair<int, size_t>, std::vector<void*>> parked;
	size_t parked_bytes = 0;
	static size_t size_class(size_t n)
	{
		size_t c = 4096;
		while (c < n)
			c <<= 1;
		return c;
	}
	void* take(int dev, size_t cls)
	{
		std::lock_guard<std::mutex> g(mu);
		auto it = parked.find({dev, cls});
		if (it == parked.end() || it->second.empty())
			return nullptr;
		void* p = it->second.back();
		it->second.pop_back();
		parked_bytes -= cls;
		return p;
	}
	bool give(int dev, size_t cls, void* p)
	{
		std::lock_guard<std::mutex> g(mu);
		if (parked_bytes + cls > kMaxParked)
			return false;
		parked[{dev, cls}].push_back(p);
		parked_bytes += cls;
		return true;
	}
	// hand everything parked for `dev` (or for every device: dev < 0) back to the runtime: called when a hipMalloc
	// fails -- a filter that nearly fills the HBM must not lose its scratch to parked staging buffers -- and by
	// btlbf_release_scratch.  The caller has the device selected.
	void drain(int dev)
	{
		std::vector<void*> out;
		{
			std::lock_guard<std::mutex> g(mu);
			for (auto& kv : parked) {
				if (dev >= 0 && kv.first.first != dev)
					continue;
				parked_bytes -= kv.first.second * kv.second.size();
				out.insert(out.end(), kv.second.begin(), kv.second.end());
				kv.second.clear();
			}
		}
		for (void* p : out)
			(void)hipFree(p);
	}
};
DevPool& dev_pool(); // the one pool of the process (capi.cpp)

template <bool kPinned>
bool GrowOnly<kPinned>::grow(uint64_t need, int device)
{
	if (need <= bytes)
		return true;
	release();
	const auto alloc = [&] { return kPinned ? hipHostMalloc(&p, need, hipHostMallocDefault) : hipMalloc(&p, need); };
	if (alloc() != hipSuccess) { // parked staging buffers of HOST-mode calls may be what is missing
		(void)hipGetLastError();
		dev_pool().drain(device);
		if (alloc() != hipSuccess) {
			(void)hipGetLastError();
			p = nullptr;
			return false;
		}
	}
	bytes = need;
	return true;
}

struct DevBuf {
	void* p = nullptr;
	size_t pooled_class = 0;
	int pooled_dev = -1;
	~DevBuf()
	{
		if (!p)
			return;
		if (pooled_class && dev_pool().give(pooled_dev, pooled_class, p))
			return;
		(void)hipFree(p);
	}
	hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 16); }
	// for buffers whose user synchronises its stream before this object dies (HOST-mode staging)
	hipError_t alloc_pooled(size_t n)
	{
		if (n > DevPool::kMaxClass || hipGetDevice(&pooled_dev) != hipSuccess)
			return alloc(n);
		const size_t cls = DevPool::size_class(n ? n : 16);
		if ((p = dev_pool().take(pooled_dev, cls)) != nullptr) {
			pooled_class = cls;
			return hipSuccess;
		}
		hipError_t e = hipMalloc(&p, cls);
		if (e != hipSuccess) { // out of memory with buffers parked: give them back and try once more
			(void)hipGetLastError();
			dev_pool().drain(pooled_dev);
			e = hipMalloc(&p, cls);
		}
		if (e == hipSuccess)
			pooled_class = cls;
		return e;
	}
	template <class T>
	T* as()
	{
		return static_cast<T*>(p);
	}
};

// A pinned, GPU-mapped mailbox per host thread for small HOST-mode calls: the kernel reads its input from and
// writes its results to it directly (zero copy), so such a call is one launch and one stream synchronisation
// instead of staging buffers and three or four copies.  Freed when its thread ends.
struct Mailbox {
	static constexpr size_t kBytes = 1u << 20;
	uint8_t* host = nullptr;
	uint8_t* dev = nullptr;
	// a thread that ends gives its pinned megabytes back (a process that starts a thread per task would otherwise pin
	// memory without bound) -- unless the HIP runtime is already shutting down: hipHostFree then fails, harmlessly
	~Mailbox()
	{
		if (host)
			(void)hipHostFree(host);
		host = dev = nullptr;
	}
	bool get()
	{
		if (host)
			return true;
		void* h = nullptr;
		if (hipHostMalloc(&h, kBytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
			(void)hipGetLastError();
			return false;
		}
		void* d = nullptr;
		if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
			(void)hipGetLastError();
			(void)hipHostFree(h);
			return false;
		}
		host = static_cast<uint8_t*>(h);
		dev = static_cast<uint8_t*>(d);
		return true;
	}
};
Mailbox& mailbox(); // the calling thread's mailbox for the current device (capi.cpp)

// parameter blocks and the filter object (capi.cpp)
void fill_hash_params(HashParams& hp, unsigned k, unsigned h);
int build_spaced(HashParams& hp, const char* const* seeds, unsigned n_seeds, unsigned h2,
                 uint64_t** d_pos, uint16_t** d_dc);
void fill_mod(ModParams& m, uint64_t size, uint64_t lo, uint64_t len);
int make_filter(btlbf_filter** out, int kind, uint64_t size, uint64_t size_bytes, unsigned shard_index,
                unsigned shard_count, unsigned h, unsigned k, unsigned thr, int device);

// device-resident view of a caller's sequence buffer (+ layout), staging host memory if needed
struct SeqView {
	DevBuf seq_buf, starts_buf;
	const uint8_t* d_seq = nullptr;
	LayoutParams lay{nullptr, 0, 0};
};

int check_layout(const btlbf_layout* l, uint64_t len);
int make_view(SeqView& v, const char* seq, uint64_t len, const btlbf_layout* l, int mem, hipStream_t s);
SeqArgs base_args(const btlbf_filter* f, const SeqView& v, uint64_t len);
int seq_precheck(const btlbf_filter* f); // host_seq.cpp
inline uint64_t bitmap_bytes(uint64_t len) { return (len + 63) / 64 * 8; }

// device view of an array of the caller's that the call writes: a pooled buffer when the call was BTLBF_HOST, copied back
// by finish() (copy_in: the call updates the array, so the caller's contents go in first)
struct OutBuf {
	DevBuf dev;
	void* host = nullptr;
	size_t n = 0;
	void* d = nullptr;
	int prepare(void* user, size_t nbytes, int mem, bool zero, hipStream_t s, bool copy_in = false)
	{
		n = nbytes;
		if (!user)
			return BTLBF_OK;
		if (mem == BTLBF_DEVICE) {
			d = user;
		} else {
			host = user;
			HIP_TRY(dev.alloc_pooled(nbytes));
			d = dev.p;
			if (copy_in && nbytes)
				HIP_TRY(hipMemcpyAsync(d, user, nbytes, hipMemcpyHostToDevice, s));
		}
		if (zero && nbytes)
			HIP_TRY(hipMemsetAsync(d, 0, nbytes, s));
		return BTLBF_OK;
	}
	int finish(hipStream_t s)
	{
		if (host && n)
			HIP_TRY(hipMemcpyAsync(host, d, n, hipMemcpyDeviceToHost, s));
		return BTLBF_OK;
	}
	template <class T>
	T* as() const
	{
		return static_cast<T*>(d);
	}
};

// ... and of a read-only array: copied in, never back
struct InBuf : private OutBuf {
	int prepare(const void* user, size_t nbytes, int mem, hipStream_t s)
	{
		return OutBuf::prepare(const_cast<void*>(user), nbytes, mem, false, s, true);
	}
	template <class T>
	const T* as() const
	{
		return static_cast<const T*>(d);
	}
};

// the sequence path enters the partitioned pipeline through these: inserts (host_partition.cpp) ...
bool want_partitioned(const btlbf_filter* f, uint64_t len, int counting_op = -1);
int partitioned_insert(btlbf_filter* f, const SeqArgs& base, hipStream_t s, bool* done);

// ... and contains() (host_query.cpp).  The ways one call can be answered: the direct kernel over the whole buffer; the
// partitioned pipeline over the whole buffer; uniform reads sampled one by one, the warm ones partitioned in place under
// a read mask and only the cold ones gathered for the direct kernel (SplitCold), or both compacted (SplitWarm)
enum class QueryRoute { Direct, Partitioned, SplitCold, SplitWarm };
// contains() of `a` by the route AUTO / the query mode picks; *answered = false: nothing was written, the caller
// launches the direct kernel `op` over the whole buffer
int contains_routed(btlbf_filter* f, const SeqArgs& a, int op, hipStream_t s, bool* answered);

// The rank structure of a whole bit filter (host_aux.cpp): *d_il gets n_blocks records of 9 uint64_t, which the caller
// owns, and *ones the popcount.  After an allocation that failed *d_il is null; after a build that failed it is not.
hipError_t rank_build(const btlbf_filter* f, uint64_t** d_il, uint64_t* n_blocks, uint64_t* ones);

// What the other miBF host units (host_mibf_probs.cpp, host_mibf_fastx.cpp) need of the object, which host_mibf.cpp keeps
// to itself: its device, its id width, the largest m_counts index over the data array -- the reduction classify caches
// until the array next changes -- and the classification of sequences that are on the device already.
int mibf_device(const btlbf_mibf* m);
unsigned mibf_id_bytes(const btlbf_mibf* m);
int mibf_max_id(btlbf_mibf* m, uint64_t* max_id);

// The offsets of a plan's batches on the device, every batch's rebased to its first byte (to the kernels a batch is a
// buffer of its own).  A plan of one batch is the whole call and uses the call's own device offsets where it has them;
// otherwise the offsets of all batches go up in one copy from pinned memory, before the first batch runs: batch i,
// sequences [s0, s1), has its s1 - s0 + 1 entries from entry s0 + i on.  The owner synchronises the stream before it goes.
struct MibfBatchStarts {
	PinScratch host;
	DevScratch dev;
	const uint64_t* d = nullptr; // batch i of the plan, sq in sequences: layout(q, sq, i)
	// per_unit: the sequences of a unit of the plan (2: pairs); d_call: the call's n_seqs + 1 offsets on the device, or null
	int stage(const MibfSeqs& q, const MibfPlan& plan, unsigned per_unit, const uint64_t* d_call, int device, hipStream_t s);
	LayoutParams layout(const MibfSeqs& q, const MibfBatch& sq, size_t i) const
	{
		return LayoutParams{q.read_len ? nullptr : d + sq.s0 + i, sq.s1 - sq.s0, q.read_len};
	}
};

// mibf_classify_device's scratch: phase 1's values, bitmaps and hit masks of the largest batch, the lists and tables of
// the sequences whose table does not fit LDS, the batches' offsets.  kept: a file's handle owns it (hence keep_room)
struct MibfClassifyScratch {
	DevScratch vals, hit, valid, masks, big_list, big_off, big_tab;
	MibfBatchStarts starts;
	bool kept = false;
	bool reserve(const MibfPlan& plan, unsigned h, unsigned id_bytes, int device);
};

// MIBFQuerySupport<T>::query of the sequences q (or, with `pairs`, of the pairs 2i, 2i + 1) of d_seq[0, len), everything
// on the device: the tables of n_ids entries, the four result arrays of a row per unit; d_starts: q's offsets, where the
// caller has them there.  Takes the miBF's lock, plans under its budget, returns with `s` synchronised (host_mibf.cpp).
int mibf_classify_device(btlbf_mibf* m, const uint8_t* d_seq, uint64_t len, const MibfSeqs& q, const uint64_t* d_starts,
                         const btlbf_mibf_classify_params& p, const double* d_prob, const uint32_t* d_minc, uint64_t n_ids,
                         btlbf_mibf_hit* d_hits, uint32_t* d_n, uint32_t* d_sat, uint32_t* d_eval, bool pairs, hipStream_t s,
                         MibfClassifyScratch& sc);

} // namespace btlbf
