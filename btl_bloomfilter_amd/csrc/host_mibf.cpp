// csrc/host_mibf.cpp -- the multi-index Bloom filter (miBF stages 2-4): the ID array over the rank structure of a bit
// filter: create, insert IDs, saturate, query, classify, statistics, files (kernels: mibf_kernels.hip,
// mibf_classify_kernels.hip, mibf_classify_pair_kernels.hip; the rank structure itself is built by rank_build,
// host_aux.cpp).  Classification has two halves: mibf_classify_device works on device-resident sequences, from their host
// offsets and with scratch its caller owns (host_mibf_fastx.cpp calls it per batch); btlbf_mibf_classify_seqs / _pairs add
// what the C ABI owes any caller: the argument checks, a HOST-mode call's staging, a DEVICE-mode caller's offsets read back.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"

#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

using namespace btlbf;

struct btlbf_mibf {
	std::mutex mu;
	int device = 0;
	unsigned id_bytes = 2, h = 0, k = 0;
	uint64_t n_bits = 0, n_blocks = 0, pop = 0;
	uint64_t budget = 0; // as set; mibf_budget() is what a call may use
	ModParams mod{};
	HashParams hp{};
	std::vector<std::string> seeds;
	uint64_t* d_il = nullptr;
	void* d_data = nullptr;   // pop T, padded to 4 bytes (the saturation OR is a 32-bit atomic)
	void* d_counts = nullptr; // pop T
	uint64_t* d_pos_tab = nullptr;
	uint16_t* d_dc_idx = nullptr;
	MibfStat* d_stat = nullptr;
	// classify: the largest m_counts index over the data array, valid until the array next changes
	bool max_id_known = false;
	uint64_t max_id = 0;
	uint64_t cls_paths[2] = {0, 0}; // the last classify call: sequences (or pairs) walked over an LDS / a global table
};

namespace {

void mibf_free(btlbf_mibf* m)
{
	if (!m)
		return;
	(void)hipFree(m->d_il);
	(void)hipFree(m->d_data);
	(void)hipFree(m->d_counts);
	(void)hipFree(m->d_pos_tab);
	(void)hipFree(m->d_dc_idx);
	(void)hipFree(m->d_stat);
	delete m;
}

uint64_t mibf_array_bytes(const btlbf_mibf* m) { return (m->pop * m->id_bytes + 3) / 4 * 4 + 4; }

// MIBloomFilter(hashNum, k, bv, seeds) + getEmptyMIBF (MIBloomFilter.hpp:122-147, MIBFConstructSupport.hpp:92-99).
// want_pop != ~0: the popcount the ID array must have (a file's size field; EFORMAT otherwise)
int mibf_make(btlbf_mibf** out, btlbf_filter* f, unsigned id_bytes, const std::vector<std::string>& seeds,
              uint64_t want_pop)
{
	if (f->kind != BTLBF_BLOOM || f->shard_count != 1)
		return fail(BTLBF_EINVAL, "miBF: needs a whole bit filter");
	if (f->h == 0 || f->h > kMibfMaxHash)
		return fail(BTLBF_EINVAL, "miBF: %u hash values per window (1..%u supported)", f->h, kMibfMaxHash);
	HashParams hp;
	fill_hash_params(hp, f->k, f->h);
	btlbf_mibf* m = new btlbf_mibf();
	m->device = f->device;
	m->id_bytes = id_bytes;
	m->h = f->h;
	m->k = f->k;
	m->seeds = seeds;
	DeviceGuard g(f->device);
	if (!seeds.empty()) {
		std::vector<const char*> sp;
		for (const auto& x : seeds)
			sp.push_back(x.c_str());
		int rc = build_spaced(hp, sp.data(), (unsigned)sp.size(), 1, &m->d_pos_tab, &m->d_dc_idx);
		if (rc) {
			mibf_free(m);
			return rc;
		}
		if (!part_supported(hp)) {
			mibf_free(m);
			return fail(BTLBF_EINVAL, "miBF: these spaced seeds leave out more than %u distinct positions", kMaxDcu);
		}
	}
	m->hp = hp;
	m->n_bits = f->size;
	fill_mod(m->mod, f->size, 0, f->size);
	hipError_t e = hipMalloc((void**)&m->d_stat, sizeof(MibfStat));
	if (e == hipSuccess)
		e = rank_build(f, &m->d_il, &m->n_blocks, &m->pop);
	if (e != hipSuccess && !m->d_il) {
		(void)hipGetLastError();
		mibf_free(m);
		return fail(BTLBF_ENOMEM, "miBF: rank structure of %llu bits", (unsigned long long)f->size);
	}
	if (e != hipSuccess) {
		mibf_free(m);
		return fail(BTLBF_EHIP, "miBF: %s", hipGetErrorString(e));
	}
	if (want_pop != ~0ull && m->pop != want_pop) {
		const unsigned long long got = m->pop;
		mibf_free(m);
		return fail(BTLBF_EFORMAT, "miBF: the bit vector has %llu set bits, the file %llu IDs", got,
		            (unsigned long long)want_pop);
	}
	e = hipMalloc(&m->d_data, mibf_array_bytes(m));
	if (e == hipSuccess)
		e = hipMalloc(&m->d_counts, mibf_array_bytes(m));
	if (e == hipSuccess)
		e = hipMemset(m->d_data, 0, mibf_array_bytes(m));
	if (e == hipSuccess)
		e = hipMemset(m->d_counts, 0, mibf_array_bytes(m));
	if (e == hipSuccess)
		e = hipDeviceSynchronize();
	if (e != hipSuccess) {
		(void)hipGetLastError();
		mibf_free(m);
		return fail(BTLBF_ENOMEM, "miBF: ID array of %llu entries", (unsigned long long)m->pop);
	}
	*out = m;
	return BTLBF_OK;
}

// the sequences of one call: device buffer, the sequence boundaries on the host (batches are cut on them), ids
struct MibfCall {
	SeqView v;
	InBuf ids;
	MibfSeqs q;
};

int mibf_prepare(MibfCall& c, const char* seq, uint64_t len, const btlbf_layout* layout, const uint32_t* ids, int mem,
                 hipStream_t s, bool want_ids = true)
{
	if (!layout || (!layout->starts && !layout->read_len))
		return fail(BTLBF_EINVAL, "miBF: a layout (read_len or starts) gives every sequence its id");
	if (!ids && want_ids)
		return fail(BTLBF_EINVAL, "miBF: null ids");
	int rc = make_view(c.v, seq, len, layout, mem, s);
	if (rc)
		return rc;
	MibfSeqs& q = c.q;
	if (layout->starts) {
		q.n_seqs = layout->n_seqs;
		q.starts.resize(q.n_seqs + 1);
		if (mem == BTLBF_DEVICE) {
			// in the order of `s`: the caller's stream may still be producing the offsets (btlbf_interleave_mates on `s`
			// writes them and returns), and a non-blocking stream is not waited for by a copy on the NULL stream
			HIP_TRY(hipMemcpyAsync(q.starts.data(), layout->starts, (q.n_seqs + 1) * 8, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
		} else
			memcpy(q.starts.data(), layout->starts, (q.n_seqs + 1) * 8);
		if (q.starts[0] != 0 || q.starts[q.n_seqs] != len)
			return fail(BTLBF_EINVAL, "starts[0] must be 0 and starts[n_seqs] must equal len");
		for (uint64_t i = 0; i < q.n_seqs; ++i)
			if (q.starts[i + 1] < q.starts[i])
				return fail(BTLBF_EINVAL, "starts must not decrease");
	} else {
		q.read_len = layout->read_len;
		q.n_seqs = len / q.read_len;
	}
	return want_ids ? c.ids.prepare(ids, q.n_seqs * 4, mem, s) : BTLBF_OK;
}

// a plan that failed: no batch has run, so the ID array, the counts and the caller's outputs are as they were
int mibf_too_big(const MibfPlan& plan, const char* unit = "sequence")
{
	return fail(BTLBF_ENOMEM, "miBF: %s %llu does not fit the scratch budget (btlbf_mibf_set_scratch); nothing was "
	            "changed", unit, (unsigned long long)plan.too_big);
}

MibfArgs mibf_args(const btlbf_mibf* m, const uint8_t* seq, uint64_t len, const LayoutParams& lay)
{
	MibfArgs a{};
	a.seq = seq;
	a.len = len;
	a.layout = lay;
	a.mod = m->mod;
	a.hp = m->hp;
	a.hp.dc_idx = m->d_dc_idx;
	a.il = m->d_il;
	a.data = m->d_data;
	a.counts_t = m->d_counts;
	return a;
}

constexpr size_t kMibfCallStat = offsetof(MibfStat, max_id);   // the four counters of a call
constexpr size_t kMibfCallStat2 = offsetof(MibfStat, mutated); // the first two: what a query and mibf_stats report

// a MIBF_QUERY launch's arguments: its outputs (hit_masks is optional) and the call counters
MibfArgs mibf_query_args(const btlbf_mibf* m, const uint8_t* seq, uint64_t len, const LayoutParams& lay, unsigned max_miss,
                         void* values, void* hit_bits, void* valid_bits, void* hit_masks)
{
	MibfArgs a = mibf_args(m, seq, len, lay);
	a.max_miss = max_miss;
	a.values = values;
	a.hit_bits = static_cast<uint8_t*>(hit_bits);
	a.valid_bits = static_cast<uint8_t*>(valid_bits);
	a.hit_masks = static_cast<uint8_t*>(hit_masks);
	a.stat = &m->d_stat->clean;
	return a;
}

// the largest m_counts index over the data array into m->max_id, cached until the array next changes; m->mu is held
int mibf_max_id_locked(btlbf_mibf* m, hipStream_t s)
{
	if (m->max_id_known)
		return BTLBF_OK;
	HIP_TRY(hipMemsetAsync(&m->d_stat->max_id, 0, sizeof(MibfStat::max_id), s));
	HIP_TRY(launch_mibf_classify_maxid(m->id_bytes, m->d_data, m->pop, &m->d_stat->max_id, s));
	unsigned long long mx = 0;
	HIP_TRY(hipMemcpyAsync(&mx, &m->d_stat->max_id, sizeof mx, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	m->max_id = mx;
	m->max_id_known = true;
	return BTLBF_OK;
}

unsigned bit_len(uint64_t x) { return x ? 64 - __builtin_clzll(x) : 0; }

#pragma pack(push, 1)
struct MibfFileHeader { // MIBloomFilter.hpp:106-117
	char magic[8];
	uint32_t hlen;
	uint64_t size;
	uint32_t nhash;
	uint32_t kmer;
	uint32_t version;
};
#pragma pack(pop)
static_assert(sizeof(MibfFileHeader) == 32, "packed miBF header");
constexpr uint32_t kMibfVersion = 1;

} // namespace

int btlbf::mibf_device(const btlbf_mibf* m) { return m->device; }
unsigned btlbf::mibf_id_bytes(const btlbf_mibf* m) { return m->id_bytes; }
int btlbf::mibf_max_id(btlbf_mibf* m, uint64_t* max_id)
{
	std::lock_guard<std::mutex> lk(m->mu);
	DeviceGuard g(m->device);
	const int rc = mibf_max_id_locked(m, nullptr);
	*max_id = m->max_id;
	return rc;
}

int btlbf::MibfBatchStarts::stage(const MibfSeqs& q, const MibfPlan& plan, unsigned per_unit, const uint64_t* d_call,
                                  int device, hipStream_t s)
{
	d = d_call;
	if (q.read_len || (plan.batches.size() == 1 && d_call))
		return BTLBF_OK;
	const uint64_t n = q.n_seqs + plan.batches.size();
	if (!host.grow(n * 8, device) || !dev.grow(n * 8, device))
		return fail(BTLBF_ENOMEM, "miBF: the batches' offsets of %llu sequences", (unsigned long long)q.n_seqs);
	uint64_t* o = host.as<uint64_t>();
	for (const MibfBatch& b : plan.batches)
		for (uint64_t i = per_unit * b.s0; i <= per_unit * b.s1; ++i)
			*o++ = q.starts[i] - q.starts[per_unit * b.s0];
	HIP_TRY(hipMemcpyAsync(dev.p, host.p, (o - host.as<uint64_t>()) * 8, hipMemcpyHostToDevice, s));
	d = dev.as<uint64_t>();
	return BTLBF_OK;
}

bool btlbf::MibfClassifyScratch::reserve(const MibfPlan& plan, unsigned h, unsigned id_bytes, int device)
{
	// never an empty buffer: a batch of empty sequences still hands the kernels pointers
	auto room = [&](DevScratch& b, uint64_t n) { return kept ? b.keep_room(n + 16, device) : b.grow(n + 16, device); };
	return room(vals, plan.max_bytes * h * id_bytes) && room(hit, bitmap_bytes(plan.max_bytes)) &&
	       room(valid, bitmap_bytes(plan.max_bytes)) && room(masks, plan.max_bytes) && room(big_list, plan.max_big * 4) &&
	       room(big_off, plan.max_big * 8) && room(big_tab, plan.max_slots * kMibfClsSlotWords * 4);
}

extern "C" int btlbf_mibf_create(btlbf_mibf** out, btlbf_filter* f, unsigned id_bytes)
{
	if (!out || !f)
		return fail(BTLBF_EINVAL, "null argument");
	*out = nullptr;
	if (id_bytes != 2 && id_bytes != 4)
		return fail(BTLBF_EINVAL, "miBF: id_bytes must be 2 or 4 (uint16_t / uint32_t IDs), not %u", id_bytes);
	FilterLock lk__(f);
	if (f->hp.n_seeds && f->hp.h2 != 1)
		return fail(BTLBF_EINVAL, "miBF: spaced seeds need h2 = 1 (MIBFQuerySupport.hpp:167-168), not %u", f->hp.h2);
	if (btlbf_device_count() <= f->device)
		return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", f->device);
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize());
	return mibf_make(out, f, id_bytes, f->hp.n_seeds ? f->seed_strs : std::vector<std::string>(), ~0ull);
}

extern "C" void btlbf_mibf_destroy(btlbf_mibf* m)
{
	if (!m)
		return;
	DeviceGuard g(m->device);
	mibf_free(m);
}

extern "C" uint64_t btlbf_mibf_size(const btlbf_mibf* m) { return m ? m->pop : 0; }
extern "C" uint64_t btlbf_mibf_bits(const btlbf_mibf* m) { return m ? m->n_bits : 0; }
extern "C" unsigned btlbf_mibf_hash_num(const btlbf_mibf* m) { return m ? m->h : 0; }
extern "C" unsigned btlbf_mibf_kmer_size(const btlbf_mibf* m) { return m ? m->k : 0; }

extern "C" int btlbf_mibf_set_scratch(btlbf_mibf* m, uint64_t bytes)
{
	if (!m)
		return fail(BTLBF_EINVAL, "null argument");
	std::lock_guard<std::mutex> lk(m->mu);
	m->budget = bytes;
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_insert_ids_seqs(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout,
                                          const uint32_t* ids, int mem, void* stream)
{
	if (!m)
		return fail(BTLBF_EINVAL, "null argument");
	std::lock_guard<std::mutex> lk(m->mu);
	DeviceGuard g(m->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	MibfCall c;
	int rc = mibf_prepare(c, seq, len, layout, ids, mem, s);
	if (rc)
		return rc;
	if (len == 0 || c.q.n_seqs == 0)
		return BTLBF_OK;
	const MibfPlan plan = mibf_plan_insert(c.q, mibf_budget(m->budget), m->h);
	if (!plan.ok())
		return mibf_too_big(plan);
	m->max_id_known = false;
	const uint64_t cap = plan.max_bytes * m->h;
	size_t temp_bytes = 0;
	HIP_TRY(mibf_sort_temp_bytes(cap, &temp_bytes));
	DevBuf kin, vin, kout, vout, temp;
	if (kin.alloc(cap * 8) || vin.alloc(cap * 8) || kout.alloc(cap * 8) || vout.alloc(cap * 8) || temp.alloc(temp_bytes)) {
		(void)hipGetLastError();
		return fail(BTLBF_ENOMEM, "miBF: %llu bytes of insert scratch", (unsigned long long)(cap * 32 + temp_bytes));
	}
	MibfBatchStarts starts;
	if ((rc = starts.stage(c.q, plan, 1, c.v.lay.starts, m->device, s)))
		return rc;
	for (const MibfBatch& b : plan.batches) {
		const uint64_t b0 = c.q.start(b.s0), blen = c.q.start(b.s1) - b0, n = blen * m->h;
		MibfArgs a = mibf_args(m, c.v.d_seq + b0, blen, starts.layout(c.q, b, &b - plan.batches.data()));
		a.seq_bits = std::max(1u, bit_len(b.s1 - b.s0 - 1));
		const unsigned end_bit = bit_len(m->pop) + a.seq_bits;
		if (end_bit > 64)
			return fail(BTLBF_EINVAL, "miBF: %llu sequences in one batch of a %llu-entry ID array",
			            (unsigned long long)(b.s1 - b.s0), (unsigned long long)m->pop);
		a.keys = kin.as<uint64_t>();
		a.vals = vin.as<uint64_t>();
		HIP_TRY(launch_mibf_seq(MIBF_EMIT, m->id_bytes, a, s));
		HIP_TRY(mibf_sort_pairs(temp.p, temp_bytes, kin.as<uint64_t>(), kout.as<uint64_t>(), vin.as<uint64_t>(),
		                        vout.as<uint64_t>(), n, end_bit, s));
		HIP_TRY(launch_mibf_insert_apply(m->id_bytes, kout.as<uint64_t>(), vout.as<uint64_t>(), n, a.seq_bits, c.ids.as<uint32_t>(), b.s0,
		                                 m->d_data, m->d_counts, s));
	}
	HIP_TRY(hipStreamSynchronize(s)); // scratch is freed on return
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_saturate_seqs(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout,
                                        const uint32_t* ids, int order, uint64_t* counts4, int mem, void* stream)
{
	if (!m)
		return fail(BTLBF_EINVAL, "null argument");
	if (order != BTLBF_ORDER_PARALLEL && order != BTLBF_ORDER_SERIAL)
		return fail(BTLBF_EINVAL, "order must be BTLBF_ORDER_PARALLEL or BTLBF_ORDER_SERIAL");
	std::lock_guard<std::mutex> lk(m->mu);
	DeviceGuard g(m->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	MibfCall c;
	int rc = mibf_prepare(c, seq, len, layout, ids, mem, s);
	if (rc)
		return rc;
	const uint64_t budget = mibf_budget(m->budget);
	m->max_id_known = false;
	HIP_TRY(hipMemsetAsync(m->d_stat, 0, kMibfCallStat, s));
	if (order == BTLBF_ORDER_SERIAL) {
		// hash rows of a batch (8 bytes per hash value + the window bitmap), then one lane in buffer order
		const MibfPlan plan = mibf_plan_serial(c.q, budget, m->h);
		if (!plan.ok())
			return mibf_too_big(plan);
		const uint64_t cap = plan.max_bytes + 64;
		DevBuf rows, valid;
		if (rows.alloc(cap * 8 * m->h) || valid.alloc(bitmap_bytes(cap))) {
			(void)hipGetLastError();
			return fail(BTLBF_ENOMEM, "miBF: serial saturation scratch");
		}
		MibfBatchStarts starts;
		if ((rc = starts.stage(c.q, plan, 1, c.v.lay.starts, m->device, s)))
			return rc;
		for (const MibfBatch& b : plan.batches) {
			const uint64_t b0 = c.q.start(b.s0), blen = c.q.start(b.s1) - b0;
			const LayoutParams lay = starts.layout(c.q, b, &b - plan.batches.data());
			SeqArgs h{};
			h.seq = c.v.d_seq + b0;
			h.len = blen;
			h.layout = lay;
			h.hp = m->hp;
			h.hp.dc_idx = m->d_dc_idx;
			fill_mod(h.mod, 8, 0, 8);
			h.hashes = rows.as<uint64_t>();
			h.valid_bits = valid.as<uint8_t>();
			HIP_TRY(launch_seq_op(OP_HASH_ONLY, h, s));
			HIP_TRY(launch_mibf_serial_saturate(m->id_bytes, rows.as<uint64_t>(), valid.as<uint64_t>(), blen, m->h, m->mod,
			                                    m->d_il, lay, c.ids.as<uint32_t>(), b.s0, m->d_data, m->d_counts, &m->d_stat->clean, s));
		}
	} else if (len) {
		// decisions against the snapshot: mutations (rank, window) 16 bytes + 16 more for their sort, saturated ranks 8
		// bytes each; half of the budget each
		const uint64_t cap_mut = mibf_parallel_cap_mut(budget), cap_sat = mibf_parallel_cap_sat(budget);
		DevBuf kin, vin, sat, cnt;
		if (kin.alloc(cap_mut * 8) || vin.alloc(cap_mut * 8) || sat.alloc(cap_sat * 8) || cnt.alloc(16)) {
			(void)hipGetLastError();
			return fail(BTLBF_ENOMEM, "miBF: %llu bytes of saturation scratch", (unsigned long long)budget);
		}
		HIP_TRY(hipMemsetAsync(cnt.p, 0, 16, s));
		MibfArgs a = mibf_args(m, c.v.d_seq, len, c.v.lay);
		a.ids = c.ids.as<uint32_t>();
		a.keys = kin.as<uint64_t>();
		a.vals = vin.as<uint64_t>();
		a.sat = sat.as<uint64_t>();
		a.cap_mut = cap_mut;
		a.cap_sat = cap_sat;
		a.n_out = cnt.as<unsigned long long>();
		a.stat = &m->d_stat->clean;
		HIP_TRY(launch_mibf_seq(MIBF_DECIDE, m->id_bytes, a, s));
		unsigned long long n_out[2];
		HIP_TRY(hipMemcpyAsync(n_out, cnt.p, 16, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (n_out[0] > cap_mut || n_out[1] > cap_sat)
			return fail(BTLBF_ENOMEM, "miBF: %llu mutations / %llu saturated positions exceed the scratch budget of "
			            "%llu bytes (btlbf_mibf_set_scratch); nothing was changed",
			            n_out[0], n_out[1], (unsigned long long)budget);
		size_t temp_bytes = 0;
		HIP_TRY(mibf_sort_temp_bytes(n_out[0], &temp_bytes));
		DevBuf kout, vout, temp;
		if (kout.alloc(n_out[0] * 8) || vout.alloc(n_out[0] * 8) || temp.alloc(temp_bytes)) {
			(void)hipGetLastError();
			return fail(BTLBF_ENOMEM, "miBF: saturation scratch");
		}
		HIP_TRY(mibf_sort_pairs(temp.p, temp_bytes, kin.as<uint64_t>(), kout.as<uint64_t>(), vin.as<uint64_t>(),
		                        vout.as<uint64_t>(), n_out[0], bit_len(m->pop), s));
		HIP_TRY(launch_mibf_mutate_apply(m->id_bytes, kout.as<uint64_t>(), vout.as<uint64_t>(), n_out[0], c.v.lay,
		                                 c.ids.as<uint32_t>(), m->d_data, m->d_counts, s));
		HIP_TRY(launch_mibf_saturate(m->id_bytes, sat.as<uint64_t>(), n_out[1], m->d_data, s));
	}
	uint64_t st[kMibfCallStat / 8];
	HIP_TRY(hipMemcpyAsync(st, m->d_stat, sizeof st, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if (counts4) {
		if (mem == BTLBF_DEVICE)
			HIP_TRY(hipMemcpy(counts4, st, sizeof st, hipMemcpyHostToDevice));
		else
			memcpy(counts4, st, sizeof st);
	}
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_query_seqs(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout,
                                     unsigned max_miss, void* values, uint64_t* match_bits, uint64_t* valid_bits,
                                     uint64_t* counts2, int mem, void* stream)
{
	if (!m || !values)
		return fail(BTLBF_EINVAL, "null argument");
	std::lock_guard<std::mutex> lk(m->mu);
	DeviceGuard g(m->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	SeqView v;
	int rc = make_view(v, seq, len, layout, mem, s);
	if (rc)
		return rc;
	OutBuf o_val, o_hit, o_valid, o_cnt;
	if ((rc = o_val.prepare(values, len * m->h * m->id_bytes, mem, false, s)) ||
	    (rc = o_hit.prepare(match_bits, bitmap_bytes(len), mem, false, s)) ||
	    (rc = o_valid.prepare(valid_bits, bitmap_bytes(len), mem, false, s)) ||
	    (rc = o_cnt.prepare(counts2, kMibfCallStat2, mem, false, s)))
		return rc;
	HIP_TRY(hipMemsetAsync(m->d_stat, 0, kMibfCallStat, s));
	HIP_TRY(launch_mibf_seq(MIBF_QUERY, m->id_bytes,
	                        mibf_query_args(m, v.d_seq, len, v.lay, max_miss, o_val.d, o_hit.d, o_valid.d, nullptr), s));
	if (o_cnt.d)
		HIP_TRY(hipMemcpyAsync(o_cnt.d, m->d_stat, kMibfCallStat2, hipMemcpyDeviceToDevice, s));
	if ((rc = o_val.finish(s)) || (rc = o_hit.finish(s)) || (rc = o_valid.finish(s)) || (rc = o_cnt.finish(s)))
		return rc;
	HIP_TRY(hipStreamSynchronize(s)); // d_stat is reused by the next call
	return BTLBF_OK;
}

// MIBFQuerySupport<T>::query of every sequence (MIBFQuerySupport.hpp:95-109) or, with `pairs`, of every pair of
// sequences 2i, 2i + 1 (:111-130): phase 1 is the MIBF_QUERY launch of btlbf_mibf_query_seqs into scratch, over the
// sequence layout either way; phase 2 the walk of mibf_classify_kernels.hip / mibf_classify_pair_kernels.hip, batch by
// batch under the budget.  A unit (a result row, an entry of the plan) is a sequence or a pair.
int btlbf::mibf_classify_device(btlbf_mibf* m, const uint8_t* d_seq, uint64_t len, const MibfSeqs& q, const uint64_t* d_starts,
                                const btlbf_mibf_classify_params& p, const double* d_prob, const uint32_t* d_minc,
                                uint64_t n_ids, btlbf_mibf_hit* d_hits, uint32_t* d_n, uint32_t* d_sat, uint32_t* d_eval,
                                bool pairs, hipStream_t s, MibfClassifyScratch& sc)
{
	std::lock_guard<std::mutex> lk(m->mu);
	DeviceGuard g(m->device);
	m->cls_paths[0] = m->cls_paths[1] = 0;
	const uint64_t n_units = pairs ? q.n_seqs / 2 : q.n_seqs, per = pairs ? 2 : 1;
	if (n_units == 0)
		return BTLBF_OK;
	if (q.start(per * n_units) > len)
		return fail(BTLBF_EINVAL, "internal error: miBF classify: offsets beyond the %llu bytes", (unsigned long long)len);
	// every index the walk will use lies inside the caller's tables
	int rc = mibf_max_id_locked(m, s);
	if (rc)
		return rc;
	if (m->max_id >= n_ids)
		return fail(BTLBF_EINVAL, "miBF classify: the ID array holds id %llu, the tables %llu entries; nothing was written",
		            (unsigned long long)m->max_id, (unsigned long long)n_ids);
	const MibfPlan plan = pairs ? mibf_plan_classify_pairs(q, mibf_budget(m->budget), m->k, m->h, m->id_bytes, n_ids)
	                            : mibf_plan_classify(q, mibf_budget(m->budget), m->k, m->h, m->id_bytes, n_ids);
	if (!plan.ok())
		return mibf_too_big(plan, pairs ? "pair" : "sequence");
	if (!sc.reserve(plan, m->h, m->id_bytes, m->device))
		return fail(BTLBF_ENOMEM, "miBF classify: scratch of %llu bytes", (unsigned long long)mibf_budget(m->budget));
	if ((rc = sc.starts.stage(q, plan, per, d_starts, m->device, s)))
		return rc;
	HIP_TRY(hipMemsetAsync(d_hits, 0, n_units * p.max_results * sizeof(btlbf_mibf_hit), s));
	HIP_TRY(hipMemsetAsync(d_n, 0, n_units * 4, s));
	HIP_TRY(hipMemsetAsync(d_sat, 0, n_units * 4, s));
	HIP_TRY(hipMemsetAsync(d_eval, 0, n_units * 4, s));
	HIP_TRY(hipMemsetAsync(m->d_stat, 0, kMibfCallStat, s));
	HIP_TRY(hipMemsetAsync(m->d_stat->cls_paths, 0, sizeof(MibfStat::cls_paths), s));
	uint64_t big0 = 0; // the batch's first entry of the plan's big lists
	for (size_t i = 0; i < plan.batches.size(); ++i) {
		const MibfBatch& b = plan.batches[i];
		const MibfBatch sq{per * b.s0, per * b.s1, b.big, b.slots}; // the batch in sequences: a plan of pairs counts pairs
		const uint64_t b0 = q.start(sq.s0), blen = q.start(sq.s1) - b0;
		const LayoutParams lay = sc.starts.layout(q, sq, i);
		if (blen)
			HIP_TRY(launch_mibf_seq(MIBF_QUERY, m->id_bytes,
			                        mibf_query_args(m, d_seq + b0, blen, lay, p.max_miss, sc.vals.p, sc.hit.p, sc.valid.p,
			                                        sc.masks.p), s));
		MibfClassifyArgs a{};
		a.values = sc.vals.p;
		a.valid_bits = sc.valid.as<uint64_t>();
		a.match_bits = sc.hit.as<uint64_t>();
		a.hit_masks = sc.masks.as<uint8_t>();
		a.layout = lay;
		a.h = m->h;
		a.k = m->k;
		a.spaced = m->hp.n_seeds ? 1 : 0;
		a.extra_frame_limit = p.extra_frame_limit;
		a.min_count = p.min_count;
		a.best_hit_agree = p.best_hit_agree;
		a.max_results = p.max_results;
		a.extra_count = p.extra_count;
		a.per_frame_prob = d_prob;
		a.min_count_per_id = d_minc;
		a.n_ids = n_ids;
		a.hits = d_hits;
		a.n_hits = d_n;
		a.sat_count = d_sat;
		a.eval_count = d_eval;
		a.row0 = b.s0;
		a.stat = m->d_stat->cls_paths;
		if (b.big) {
			HIP_TRY(hipMemcpyAsync(sc.big_list.p, &plan.big_seq[big0], b.big * 4, hipMemcpyHostToDevice, s));
			HIP_TRY(hipMemcpyAsync(sc.big_off.p, &plan.big_off[big0], b.big * 8, hipMemcpyHostToDevice, s));
			HIP_TRY(hipStreamSynchronize(s)); // an early return frees the plan
			big0 += b.big;
			a.big_list = sc.big_list.as<uint32_t>();
			a.big_off = sc.big_off.as<uint64_t>();
			a.big_tab = sc.big_tab.as<uint32_t>();
			a.n_big = b.big;
		}
		HIP_TRY(pairs ? launch_mibf_classify_pairs(m->id_bytes, a, s) : launch_mibf_classify(m->id_bytes, a, s));
	}
	unsigned long long paths[2] = {0, 0};
	HIP_TRY(hipMemcpyAsync(paths, m->d_stat->cls_paths, sizeof paths, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s)); // d_stat is reused by the next call, and the scratch may go with the caller
	memcpy(m->cls_paths, paths, sizeof paths);
	return BTLBF_OK;
}

// the C entry points' half: the checks, the staging and read-back of mibf_prepare, tables and results of a HOST-mode call
static int mibf_classify(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout,
                         const btlbf_mibf_classify_params* p, const double* per_frame_prob,
                         const uint32_t* min_count_per_id, uint64_t n_ids, btlbf_mibf_hit* hits, uint32_t* n_hits,
                         uint32_t* sat_count, uint32_t* eval_count, int mem, void* stream, bool pairs)
{
	if (!m || (!seq && len) || !layout || !p || !per_frame_prob || !min_count_per_id || !hits || !n_hits || !sat_count ||
	    !eval_count)
		return fail(BTLBF_EINVAL, "null argument");
	if (p->max_results == 0)
		return fail(BTLBF_EINVAL, "miBF classify: max_results must be at least 1");
	if (n_ids == 0)
		return fail(BTLBF_EINVAL, "miBF classify: n_ids must be at least 1");
	if (pairs && ((layout->starts ? layout->n_seqs : layout->read_len ? len / layout->read_len : 0) & 1))
		return fail(BTLBF_EINVAL, "miBF classify: pairs need an even number of sequences (mate 1, mate 2, ...); nothing "
		            "was written");
	if (n_ids > (1ull << (m->id_bytes * 8 - 1)))
		return fail(BTLBF_EINVAL, "miBF classify: n_ids must be 1..2^%u for %u-byte ids, not %llu", m->id_bytes * 8 - 1,
		            m->id_bytes, (unsigned long long)n_ids);
	DeviceGuard g(m->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	MibfCall c;
	int rc = mibf_prepare(c, seq, len, layout, nullptr, mem, s, false);
	if (rc)
		return rc;
	const uint64_t n_units = pairs ? c.q.n_seqs / 2 : c.q.n_seqs;
	InBuf prob, minc;
	OutBuf o_hits, o_n, o_sat, o_eval;
	if ((rc = prob.prepare(per_frame_prob, n_ids * 8, mem, s)) || (rc = minc.prepare(min_count_per_id, n_ids * 4, mem, s)) ||
	    (rc = o_hits.prepare(hits, n_units * p->max_results * sizeof(btlbf_mibf_hit), mem, false, s)) ||
	    (rc = o_n.prepare(n_hits, n_units * 4, mem, false, s)) || (rc = o_sat.prepare(sat_count, n_units * 4, mem, false, s)) ||
	    (rc = o_eval.prepare(eval_count, n_units * 4, mem, false, s)))
		return rc;
	MibfClassifyScratch sc;
	if ((rc = mibf_classify_device(m, c.v.d_seq, len, c.q, c.v.lay.starts, *p, prob.as<double>(), minc.as<uint32_t>(), n_ids,
	                               o_hits.as<btlbf_mibf_hit>(), o_n.as<uint32_t>(), o_sat.as<uint32_t>(),
	                               o_eval.as<uint32_t>(), pairs, s, sc)) ||
	    (rc = o_hits.finish(s)) || (rc = o_n.finish(s)) || (rc = o_sat.finish(s)) || (rc = o_eval.finish(s)))
		return rc;
	HIP_TRY(hipStreamSynchronize(s)); // the staging buffers go back to the pool on return
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_classify_seqs(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout,
                                        const btlbf_mibf_classify_params* p, const double* per_frame_prob,
                                        const uint32_t* min_count_per_id, uint64_t n_ids, btlbf_mibf_hit* hits,
                                        uint32_t* n_hits, uint32_t* sat_count, uint32_t* eval_count, int mem, void* stream)
{
	return mibf_classify(m, seq, len, layout, p, per_frame_prob, min_count_per_id, n_ids, hits, n_hits, sat_count,
	                     eval_count, mem, stream, false);
}

extern "C" int btlbf_mibf_classify_pairs(btlbf_mibf* m, const char* seq, uint64_t len, const btlbf_layout* layout,
                                         const btlbf_mibf_classify_params* p, const double* per_frame_prob,
                                         const uint32_t* min_count_per_id, uint64_t n_ids, btlbf_mibf_hit* hits,
                                         uint32_t* n_hits, uint32_t* sat_count, uint32_t* eval_count, int mem, void* stream)
{
	return mibf_classify(m, seq, len, layout, p, per_frame_prob, min_count_per_id, n_ids, hits, n_hits, sat_count,
	                     eval_count, mem, stream, true);
}

extern "C" int btlbf_mibf_classify_paths(btlbf_mibf* m, uint64_t* out2)
{
	if (!m || !out2)
		return fail(BTLBF_EINVAL, "null argument");
	std::lock_guard<std::mutex> lk(m->mu);
	memcpy(out2, m->cls_paths, sizeof m->cls_paths);
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_stats(btlbf_mibf* m, uint64_t* out3)
{
	if (!m || !out3)
		return fail(BTLBF_EINVAL, "null argument");
	std::lock_guard<std::mutex> lk(m->mu);
	DeviceGuard g(m->device);
	HIP_TRY(hipMemset(m->d_stat, 0, kMibfCallStat2));
	HIP_TRY(launch_mibf_stats(m->id_bytes, m->d_data, m->pop, &m->d_stat->clean, nullptr));
	uint64_t st[2];
	HIP_TRY(hipMemcpy(st, m->d_stat, kMibfCallStat2, hipMemcpyDeviceToHost));
	out3[0] = m->pop;
	out3[1] = st[0];
	out3[2] = st[1];
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_id_counts(btlbf_mibf* m, uint64_t* counts, uint64_t n_ids, uint64_t* saturated)
{
	if (!m || (n_ids && !counts))
		return fail(BTLBF_EINVAL, "null argument");
	uint64_t st[3];
	int rc = btlbf_mibf_stats(m, st);
	if (rc)
		return rc;
	if (saturated)
		*saturated = st[2];
	if (!n_ids)
		return BTLBF_OK;
	std::lock_guard<std::mutex> lk(m->mu);
	DeviceGuard g(m->device);
	DevBuf bins;
	HIP_TRY(bins.alloc(n_ids * 8));
	HIP_TRY(hipMemset(bins.p, 0, n_ids * 8));
	HIP_TRY(launch_mibf_hist(m->id_bytes, m->d_data, m->pop, n_ids, bins.as<unsigned long long>(), nullptr));
	std::vector<uint64_t> h(n_ids);
	HIP_TRY(hipMemcpy(h.data(), bins.p, n_ids * 8, hipMemcpyDeviceToHost));
	for (uint64_t i = 0; i < n_ids; ++i)
		counts[i] += h[i];
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_download(btlbf_mibf* m, void* host_dst)
{
	if (!m || (m->pop && !host_dst))
		return fail(BTLBF_EINVAL, "null argument");
	std::lock_guard<std::mutex> lk(m->mu);
	DeviceGuard g(m->device);
	HIP_TRY(hipMemcpy(host_dst, m->d_data, m->pop * m->id_bytes, hipMemcpyDeviceToHost));
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_upload(btlbf_mibf* m, const void* host_src)
{
	if (!m || (m->pop && !host_src))
		return fail(BTLBF_EINVAL, "null argument");
	std::lock_guard<std::mutex> lk(m->mu);
	DeviceGuard g(m->device);
	m->max_id_known = false;
	HIP_TRY(hipMemcpy(m->d_data, host_src, m->pop * m->id_bytes, hipMemcpyHostToDevice));
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_download_counts(btlbf_mibf* m, void* host_dst)
{
	if (!m || (m->pop && !host_dst))
		return fail(BTLBF_EINVAL, "null argument");
	std::lock_guard<std::mutex> lk(m->mu);
	DeviceGuard g(m->device);
	HIP_TRY(hipMemcpy(host_dst, m->d_counts, m->pop * m->id_bytes, hipMemcpyDeviceToHost));
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_store(btlbf_mibf* m, const char* path)
{
	if (!m || !path)
		return fail(BTLBF_EINVAL, "null argument");
	std::vector<uint8_t> body(m->pop * m->id_bytes);
	int rc = btlbf_mibf_download(m, body.data());
	if (rc)
		return rc;
	MibfFileHeader hd;
	memcpy(hd.magic, "MIBLOOMF", 8);
	hd.hlen = (uint32_t)(sizeof hd + m->k * m->seeds.size());
	hd.size = m->pop;
	hd.nhash = m->h;
	hd.kmer = m->k;
	hd.version = kMibfVersion;
	FILE* fp = fopen(path, "wb");
	if (!fp)
		return fail(BTLBF_EIO, "error: `%s': %s", path, strerror(errno));
	bool ok = fwrite(&hd, sizeof hd, 1, fp) == 1;
	for (const auto& sd : m->seeds)
		ok = ok && fwrite(sd.data(), 1, m->k, fp) == m->k;
	ok = ok && (body.empty() || fwrite(body.data(), 1, body.size(), fp) == body.size());
	ok = (fclose(fp) == 0) && ok;
	if (!ok)
		return fail(BTLBF_EIO, "error: `%s': write failed", path);
	return BTLBF_OK;
}

extern "C" int btlbf_mibf_load(btlbf_mibf** out, const char* path, btlbf_filter* f, unsigned id_bytes)
{
	if (!out || !path || !f)
		return fail(BTLBF_EINVAL, "null argument");
	*out = nullptr;
	if (id_bytes != 2 && id_bytes != 4)
		return fail(BTLBF_EINVAL, "miBF: id_bytes must be 2 or 4 (uint16_t / uint32_t IDs), not %u", id_bytes);
	// the checks of MIBloomFilter(path) (MIBloomFilter.hpp:149-248), all before the GPU is touched
	FILE* fp = fopen(path, "rb");
	if (!fp)
		return fail(BTLBF_EIO, "file \"%s\" could not be read: %s", path, strerror(errno));
	MibfFileHeader hd;
	std::vector<std::string> seeds;
	std::vector<uint8_t> body;
	int rc = BTLBF_OK;
	if (fread(&hd, sizeof hd, 1, fp) != 1) {
		rc = fail(BTLBF_EFORMAT, "%s: Failed to Load header", path);
	} else if (memcmp(hd.magic, "MIBLOOMF", 8) != 0) {
		rc = fail(BTLBF_EFORMAT, "%s: Bloom Filter type does not match", path);
	} else {
		if (hd.hlen > sizeof hd) {
			for (unsigned i = 0; i < hd.nhash && !rc; ++i) {
				std::string sd(hd.kmer, '\0');
				if (hd.kmer > 4096 || fread(&sd[0], 1, hd.kmer, fp) != hd.kmer)
					rc = fail(BTLBF_EFORMAT, "%s: Failed to load spaced seed string", path);
				seeds.push_back(sd);
			}
		}
		if (!rc && hd.hlen != sizeof hd + (uint64_t)hd.kmer * seeds.size())
			rc = fail(BTLBF_EFORMAT, "%s: Multi Index Bloom Filter header length: %u does not match expected length",
			          path, hd.hlen);
		if (!rc && hd.version != kMibfVersion)
			rc = fail(BTLBF_EFORMAT, "%s: Multi Index Bloom Filter version does not match: %u expected: %u", path,
			          hd.version, kMibfVersion);
		if (!rc) {
			const long cur = ftell(fp);
			fseek(fp, 0, SEEK_END);
			const uint64_t file_size = (uint64_t)ftell(fp) - hd.hlen;
			fseek(fp, cur, SEEK_SET);
			if (file_size != hd.size * id_bytes)
				rc = fail(BTLBF_EFORMAT, "%s does not match size given by its header. Size: %llu vs %llu bytes.", path,
				          (unsigned long long)file_size, (unsigned long long)(hd.size * id_bytes));
		}
		if (!rc) {
			body.resize(hd.size * id_bytes);
			if (!body.empty() && fread(body.data(), 1, body.size(), fp) != body.size())
				rc = fail(BTLBF_EIO, "file \"%s\" could not be read.", path);
		}
	}
	fclose(fp);
	if (rc)
		return rc;
	FilterLock lk__(f);
	if (f->h != hd.nhash || f->k != hd.kmer)
		return fail(BTLBF_EFORMAT, "miBF: the file has %u hashes of k = %u, the bit filter %u of k = %u", hd.nhash,
		            hd.kmer, f->h, f->k);
	if (btlbf_device_count() <= f->device)
		return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", f->device);
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize());
	btlbf_mibf* m = nullptr;
	if ((rc = mibf_make(&m, f, id_bytes, seeds, hd.size)))
		return rc;
	if (!body.empty() && hipMemcpy(m->d_data, body.data(), body.size(), hipMemcpyHostToDevice) != hipSuccess) {
		mibf_free(m);
		return fail(BTLBF_EHIP, "miBF: upload failed");
	}
	*out = m;
	return BTLBF_OK;
}
