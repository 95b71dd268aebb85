// csrc/host_algebra.cpp -- the filter algebra of the C ABI: btlbf_clone, btlbf_combine (union / intersect / subtract of
// bit filters, add / max / min of counting filters), btlbf_fold and btlbf_threshold_bits (kernels: algebra_kernels.hip;
// the fold's plan: fold_plan.hpp).  Every refusal comes before the first HIP call (btlbf_set_error, not fail).
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"
#include "fold_plan.hpp"

#include <algorithm>
#include <vector>

using namespace btlbf;

namespace {

// a filter this call made and has not handed out yet
struct NewFilter {
	btlbf_filter* f = nullptr;
	~NewFilter() { (void)btlbf_destroy(f); }
	btlbf_filter* release()
	{
		btlbf_filter* r = f;
		f = nullptr;
		return r;
	}
};

// several filters locked in address order (btlbf_compare's rule for two), each once
struct MultiLock {
	std::vector<const btlbf_filter*> fs;
	explicit MultiLock(std::vector<const btlbf_filter*> all)
	  : fs(std::move(all))
	{
		std::sort(fs.begin(), fs.end());
		fs.erase(std::unique(fs.begin(), fs.end()), fs.end());
		for (const btlbf_filter* f : fs)
			f->mu.lock();
	}
	~MultiLock()
	{
		for (auto it = fs.rbegin(); it != fs.rend(); ++it)
			(*it)->mu.unlock();
	}
	MultiLock(const MultiLock&) = delete;
	MultiLock& operator=(const MultiLock&) = delete;
};

// what a derived filter takes over from `f` besides its geometry: the spaced seeds, and (with_entries) the header's counts
int take_over(btlbf_filter* nf, const btlbf_filter* f, bool with_entries)
{
	nf->bits_per_counter = f->bits_per_counter;
	if (with_entries) {
		nf->n_entry = f->n_entry;
		nf->t_entry = f->t_entry;
		nf->dfpr = f->dfpr;
	}
	if (f->hp.n_seeds == 0)
		return BTLBF_OK;
	std::vector<const char*> seeds;
	for (const std::string& s : f->seed_strs)
		seeds.push_back(s.c_str());
	return btlbf_set_spaced_seeds(nf, seeds.data(), (unsigned)seeds.size(), f->hp.h2);
}

const char* const kOpNames[] = {"OR", "AND", "ANDNOT", "ADD", "MAX", "MIN"};

// the body of btlbf_clone, with f locked
int clone_locked(btlbf_filter** out, btlbf_filter* f)
{
	NewFilter nf;
	int rc = make_filter(&nf.f, f->kind, f->size, f->size_bytes, f->shard_index, f->shard_count, f->h, f->k, f->thr, f->device);
	if (rc)
		return rc;
	if ((rc = take_over(nf.f, f, true)))
		return rc;
	if (!f->lazy_zero) { // (a cleared source: the new filter is cleared already)
		DeviceGuard g(f->device);
		MATERIALIZE(f, nullptr);
		HIP_TRY(hipDeviceSynchronize()); // DEVICE-mode calls may have run on non-blocking user streams
		HIP_TRY(hipMemcpy(nf.f->d_data, f->d_data, f->alloc_bytes, hipMemcpyDeviceToDevice));
		HIP_TRY(hipDeviceSynchronize());
		nf.f->lazy_zero = false;
	}
	*out = nf.release();
	return BTLBF_OK;
}

} // namespace

extern "C" int btlbf_clone(btlbf_filter** out, btlbf_filter* f)
{
	if (out)
		*out = nullptr;
	if (!out || !f)
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_clone: null argument");
	FilterLock lk__(f);
	return clone_locked(out, f);
}

extern "C" int btlbf_combine(btlbf_filter* dst, btlbf_filter* const* srcs, unsigned n_srcs, int op, uint64_t* pop_out)
{
	if (!dst || !srcs)
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: null argument");
	if (n_srcs == 0 || n_srcs > BTLBF_COMBINE_MAX_SRCS)
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: n_srcs must be 1..%d, not %u", BTLBF_COMBINE_MAX_SRCS, n_srcs);
	for (unsigned j = 0; j < n_srcs; ++j) {
		if (!srcs[j])
			return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: source %u is a null handle", j);
		if (srcs[j] == dst)
			return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: dst is among the sources (source %u)", j);
	}
	if (op < BTLBF_COMBINE_OR || op > BTLBF_COMBINE_MIN || (op >= BTLBF_COMBINE_ADD) != is_counting(dst))
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: op %d%s%s does not belong to a %s filter (bit filters: OR, AND, "
		                                     "ANDNOT; counting filters: ADD, MAX, MIN)",
		                       op, op >= 0 && op <= BTLBF_COMBINE_MIN ? " = " : "",
		                       op >= 0 && op <= BTLBF_COMBINE_MIN ? kOpNames[op] : "", is_counting(dst) ? "counting" : "bit");
	std::vector<const btlbf_filter*> all(srcs, srcs + n_srcs);
	all.push_back(dst);
	MultiLock lk__(all);
	for (unsigned j = 0; j < n_srcs; ++j) {
		const btlbf_filter* f = srcs[j];
		if (f->kind != dst->kind)
			return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: source %u is of kind %d, dst of kind %d", j, f->kind, dst->kind);
		if (f->size != dst->size || f->local_bytes != dst->local_bytes)
			return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: source %u differs from dst in size (%llu positions in %llu "
			                                     "local bytes, dst %llu in %llu)",
			                       j, (unsigned long long)f->size, (unsigned long long)f->local_bytes,
			                       (unsigned long long)dst->size, (unsigned long long)dst->local_bytes);
		if (f->shard_index != dst->shard_index || f->shard_count != dst->shard_count || f->mod.shard_lo != dst->mod.shard_lo)
			return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: source %u is shard %u of %u, dst is shard %u of %u", j,
			                       f->shard_index, f->shard_count, dst->shard_index, dst->shard_count);
		if (f->device != dst->device)
			return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: source %u is on device %d, dst on device %d", j, f->device,
			                       dst->device);
		if (f->h != dst->h)
			return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: source %u has hash_num %u, dst %u", j, f->h, dst->h);
		if (f->k != dst->k)
			return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: source %u has kmer_size %u, dst %u", j, f->k, dst->k);
		if (f->hp.n_seeds != dst->hp.n_seeds || f->hp.h2 != dst->hp.h2 || f->seed_strs != dst->seed_strs)
			return btlbf_set_error(BTLBF_EINVAL, "btlbf_combine: source %u and dst differ in their spaced seeds", j);
	}
	DeviceGuard g(dst->device);
	if (!g.ok)
		return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", dst->device);
	CombineSrcs ptrs{};
	MATERIALIZE(dst, nullptr);
	for (unsigned j = 0; j < n_srcs; ++j) {
		MATERIALIZE(srcs[j], nullptr);
		ptrs.p[j] = srcs[j]->d_data;
	}
	HIP_TRY(hipDeviceSynchronize()); // whatever streams the filters were last used on
	HIP_TRY(hipMemset(dst->d_scalar, 0, 8));
	HIP_TRY(launch_combine((int)counter_bytes(dst), op, dst->d_data, ptrs, n_srcs, dst->alloc_bytes, dst->d_scalar, nullptr));
	unsigned long long pop = 0;
	HIP_TRY(hipMemcpy(&pop, dst->d_scalar, 8, hipMemcpyDeviceToHost)); // (waits for the kernel)
	if (pop_out)
		*pop_out = pop;
	return BTLBF_OK;
}

extern "C" int btlbf_fold(btlbf_filter** out, btlbf_filter* f, uint64_t factor)
{
	if (out)
		*out = nullptr;
	if (!out || !f)
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_fold: null argument");
	FilterLock lk__(f);
	if (f->shard_count != 1)
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_fold: needs a whole filter, not a shard");
	const unsigned cb = counter_bytes(f);
	const FoldPlan plan = fold_plan(f->size_bytes, factor, cb);
	switch (plan.refusal) {
	case kFoldOk: break;
	case kFoldFactorZero: return btlbf_set_error(BTLBF_EINVAL, "btlbf_fold: factor must be at least 1");
	case kFoldNotDivisible:
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_fold: factor %llu does not divide the filter's size %llu",
		                       (unsigned long long)factor, (unsigned long long)f->size);
	case kFoldResultNotConstructible:
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_fold: a filter of %llu / %llu = %llu %s is not a multiple of 8 %s, which no "
		                                     "constructor makes",
		                       (unsigned long long)f->size, (unsigned long long)factor, (unsigned long long)plan.out_positions,
		                       cb ? "counters" : "bits", cb ? "bytes" : "bits");
	}
	if (factor == 1)
		return clone_locked(out, f);
	NewFilter nf;
	int rc = make_filter(&nf.f, f->kind, plan.out_positions, plan.out_bytes, 0, 1, f->h, f->k, f->thr, f->device);
	if (rc)
		return rc;
	if ((rc = take_over(nf.f, f, true)))
		return rc;
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize()); // DEVICE-mode calls may have run on non-blocking user streams
	DevBuf scratch;
	if (plan.groups > 1) { // stage 1: runs of slices into the rows of a scratch; stage 2: the rows
		HIP_TRY(scratch.alloc(plan.scratch_bytes));
		HIP_TRY(launch_fold((int)cb, f->d_data, plan.out_bytes, plan.out_bytes, factor, plan.per_group, plan.groups, scratch.p,
		                    plan.out_alloc, nullptr));
		HIP_TRY(launch_fold((int)cb, scratch.p, plan.out_alloc, plan.out_alloc, plan.groups, plan.groups, 1, nf.f->d_data,
		                    plan.out_alloc, nullptr));
	} else {
		HIP_TRY(launch_fold((int)cb, f->d_data, plan.out_bytes, plan.out_bytes, factor, factor, 1, nf.f->d_data, plan.out_alloc,
		                    nullptr));
	}
	HIP_TRY(hipDeviceSynchronize());
	nf.f->lazy_zero = false; // every byte of the array was written, its padding with zeros
	*out = nf.release();
	return BTLBF_OK;
}

extern "C" int btlbf_threshold_bits(btlbf_filter** out, btlbf_filter* f, unsigned threshold)
{
	if (out)
		*out = nullptr;
	if (!out || !f)
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_threshold_bits: null argument");
	FilterLock lk__(f);
	if (!is_counting(f))
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_threshold_bits: needs a counting filter, not a bit filter");
	if (f->shard_count != 1)
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_threshold_bits: needs a whole filter, not a shard");
	const unsigned thr = threshold ? threshold : f->thr;
	if (thr == 0)
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_threshold_bits: threshold 0, and the filter's own threshold is 0 too");
	if (f->size % 8)
		return btlbf_set_error(BTLBF_EINVAL, "btlbf_threshold_bits: %llu counters are not a multiple of 8, so they make no "
		                                     "bit filter",
		                       (unsigned long long)f->size);
	NewFilter nf;
	int rc = make_filter(&nf.f, BTLBF_BLOOM, f->size, f->size / 8, 0, 1, f->h, f->k, 0, f->device);
	if (rc)
		return rc;
	if ((rc = take_over(nf.f, f, false)))
		return rc;
	nf.f->bits_per_counter = 8;
	DeviceGuard g(f->device);
	MATERIALIZE(f, nullptr);
	HIP_TRY(hipDeviceSynchronize()); // DEVICE-mode calls may have run on non-blocking user streams
	HIP_TRY(launch_threshold_bits((int)counter_bytes(f), f->d_data, f->alloc_bytes, thr, nf.f->d_data, nf.f->alloc_bytes / 8,
	                              nullptr));
	HIP_TRY(hipDeviceSynchronize());
	nf.f->lazy_zero = false; // every word of the array was written, its padding with zeros
	*out = nf.release();
	return BTLBF_OK;
}
