// csrc/host_query.cpp -- how one contains() over a sequence buffer chooses its path, and the paths that are more than
// one launch of the direct kernel.
//
// contains_routed is the entry (host_seq.cpp's run_query_like calls it and launches the direct kernel over the whole
// buffer where it was not answered).  decide_route makes the decision, once: it holds every sampling launch and every
// host read-back that steers the path and returns a QueryDecision; the executors below it carry a route out and take
// nothing back.  A route that cannot run -- no room for its scratch -- is downgraded in contains_routed's switch.
// The planner's rules and the partitioned executor (part_query) come from host_partition.cpp through
// host_partition.hpp; the split query's kernels are split_query_kernels.hip.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"
#include "host_partition.hpp"

#include <algorithm>

using namespace btlbf;

namespace {

// ---- the split query: contains() over fixed-length reads in AUTO mode (split_query_kernels.hip) ----------------------
// what its steps share: the reads' cold flags and their prefix sums (in f->flags) and the counts
struct SplitState {
	uint32_t L = 0; // read length
	uint64_t n_reads = 0;
	unsigned long long n_cold = 0, *d_ncold = nullptr;
	uint64_t* d_flags = nullptr;
	uint32_t* d_prefix = nullptr;
};

// what decide_route found: the route, and for the two split routes every read's flag and the cold count (`split`);
// SplitCold: the level-0 plan the route was chosen with, which its partitioned query takes over
struct QueryDecision {
	QueryRoute route = QueryRoute::Direct;
	SplitState split;
	PartPlan level0;
};

uint64_t up256(uint64_t x) { return (x + 255) / 256 * 256; }

// Can the reads be sampled one by one?  Uniform reads of a whole filter in AUTO mode, in a batch worth a sweep; `st`
// then has the read geometry and its flag arrays in f->flags.  false: the 64-tile sample decides.
bool split_applies(btlbf_filter* f, const SeqArgs& a, SplitState& st)
{
	const uint32_t L = a.layout.starts ? 0 : a.layout.read_len, k = f->hp.k;
	// whole filters only: the sampler probes f->d_data with positions of the whole array (a shard answers for its
	// window through the WINDOW kernels)
	if (f->shard_count != 1 || f->mod.shard_lo != 0 || f->mod.shard_len != f->mod.size)
		return false;
	if (f->query_mode != BTLBF_INSERT_AUTO || !L || L < k || L < 8 || f->hp.n_seeds || !part_supported(f->hp))
		return false;
	const uint64_t n_reads = a.len / L;
	const uint32_t W = L - k + 1;
	if (!worth_sweep(f, (double)n_reads * W * f->hp.h, kAutoQueryRatio) || n_reads >= (1ull << 32))
		return false; // small batches: the direct kernel (the 64-tile sample's first rule agrees)
	const uint64_t n_fw = (n_reads + 63) / 64;
	// temporaries are cached in the filter (DevScratch): the small one (flags, prefix sums) is needed by every call,
	// the large one (compacted reads, their bitmaps) only once a split route is taken
	// (the flags are readable for 256 bytes behind their last word: pass A reads up to 34 words from a tile's first one on)
	const uint64_t sz_flags = up256(n_fw * 8 + 256), sz_prefix = up256((n_fw + (n_fw + 1023) / 1024 + 1) * 4);
	if (!f->flags.grow(256 + sz_flags + sz_prefix, f->device))
		return false; // no room
	uint8_t* const base = static_cast<uint8_t*>(f->flags.p);
	st.L = L;
	st.n_reads = n_reads;
	st.d_ncold = reinterpret_cast<unsigned long long*>(base);
	st.d_flags = reinterpret_cast<uint64_t*>(base + 256);
	st.d_prefix = reinterpret_cast<uint32_t*>(base + 256 + sz_flags);
	return true;
}

// The decision.  Uniform reads in AUTO mode (split_applies) are sampled read by read: few misses -> Partitioned, warm
// reads not worth a sweep -> Direct, else one of the split routes.  Everything else -- shards, ragged layouts, spaced
// seeds, a forced mode, small batches -- goes by the mode and, in AUTO, by a sample of 64 tiles: Partitioned or Direct.
int decide_route(btlbf_filter* f, const SeqArgs& a, hipStream_t s, QueryDecision& d)
{
	d.route = QueryRoute::Direct;
	SplitState& st = d.split;
	if (split_applies(f, a, st)) {
		const uint32_t L = st.L, W = L - f->hp.k + 1;
		const uint64_t n_reads = st.n_reads;
		// what the fail list copes with / what is worth a sweep of the array, in reads
		// (the list the partitioned path will really have: a small scratch budget gets a short one, part_tail)
		const double few_cold = 0.25 * (double)part_tail(scratch_budget(f)).fail_cap / ((double)W * f->hp.h);
		auto sample = [&](uint32_t stride, uint32_t probes2) -> int { // flags and st.n_cold from every stride-th read
			HIP_TRY(hipMemsetAsync(st.d_ncold, 0, 8, s));
			{
				ProfSpan ps(f, BTLBF_PROF_QUERY_RESOLVE, s);
				HIP_TRY(launch_read_sample(a.seq, n_reads, L, stride, f->hp, f->mod, f->d_data, f->kind == BTLBF_COUNTING8,
				                           f->thr, st.d_flags, reinterpret_cast<uint64_t*>(st.d_ncold), s, probes2));
			}
			HIP_TRY(hipMemcpyAsync(&st.n_cold, st.d_ncold, 8, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			return BTLBF_OK;
		};
		auto warm_too_few = [&](double n_warm_reads) { return !worth_sweep(f, n_warm_reads * W * f->hp.h, kAutoQueryRatio); };
		// 1. an estimate from one read in 64: all-hit and all-miss buffers -- the common cases -- are recognised at
		//    1/64 of the cost of looking at every read
		const uint32_t stride = n_reads >= (1u << 20) ? 64 : 1;
		double cold_frac = 1.0; // estimate from the first look (unknown: assume many)
		if (stride > 1) {
			if (int rc = sample(stride, 0))
				return rc;
			const uint64_t n_s = (n_reads + stride - 1) / stride;
			cold_frac = (double)st.n_cold / (double)n_s;
			if (st.n_cold == 0 && (double)n_reads * 8.0 / (double)n_s < few_cold) { // none in the sample: few overall
				d.route = QueryRoute::Partitioned;
				return BTLBF_OK;
			}
			if (warm_too_few((double)(n_s - st.n_cold) * stride * 1.5))
				return BTLBF_OK; // Direct
		}
		// 2. every read.  A present read costs the sampler its probes (they all hit, so they are all loaded), and the second
		//    sample only has to keep a foreign read from passing on ONE false-positive window: with few foreign reads, fewer
		//    of its probes do (a read that passes all the same costs a resolve pass, never a wrong answer)
		const uint32_t h = f->hp.h;
		const uint32_t probes2 = cold_frac <= 0.0025 ? (h + 1) / 2 : cold_frac <= 0.025 ? std::max((h + 1) / 2, h - 1) : h;
		if (int rc = sample(1, probes2))
			return rc;
		if ((double)st.n_cold < few_cold) // the fail list copes with that many misses
			d.route = QueryRoute::Partitioned;
		else if (warm_too_few((double)(n_reads - st.n_cold)))
			d.route = QueryRoute::Direct;
		else {
			// the warm reads stay in place (SplitCold) with up to a quarter of the reads cold: beyond that the lanes pass A
			// spends on zero-staged reads cost more than gathering the warm reads costs -- at one read in two 76 instead
			// of 43 ms of pass A per 10^8 reads.  Level 0 is planned here, once: SplitCold's partitioned query takes it
			// over (the read grid belongs to its geometry)
			PartGrid g;
			const bool in_place = 4 * st.n_cold <= n_reads && plan_level0(f, d.level0, call_probes(f, a.len)) &&
			                      part_read_grid(f->hp, d.level0.lv[0].P, a.layout, &g);
			d.route = in_place ? QueryRoute::SplitCold : QueryRoute::SplitWarm;
		}
		return BTLBF_OK;
	}
	if (f->query_mode == BTLBF_INSERT_DIRECT)
		return BTLBF_OK;
	if (!part_supported(f->hp) || a.len == 0)
		return BTLBF_OK;
	if (f->query_mode == BTLBF_INSERT_PARTITIONED) {
		d.route = QueryRoute::Partitioned;
		return BTLBF_OK;
	}
	// AUTO: a large batch, and a sample of tiles says nearly every k-mer hits
	const double live = local_probes(f, a.len);
	if (!worth_sweep(f, live, kAutoQueryRatio))
		return BTLBF_OK;
	// sample 64 tiles spread over the buffer with the direct kernel
	const uint64_t tiles = (a.len + seq_tile_windows() - 1) / seq_tile_windows();
	const unsigned n_s = (unsigned)std::min<uint64_t>(64, tiles);
	HIP_TRY(hipMemsetAsync(f->d_scalar, 0, 16, s));
	for (unsigned i = 0; i < n_s; ++i) {
		SeqArgs t = a;
		t.first_tile = (tiles / n_s) * i;
		t.n_tiles = 1;
		t.hit_bits = nullptr;
		t.valid_bits = nullptr;
		t.counts = reinterpret_cast<uint64_t*>(f->d_scalar);
		t.min_out = nullptr;
		HIP_TRY(launch_seq_op(direct_query_op(f), t, s));
	}
	unsigned long long c[2] = {0, 0};
	HIP_TRY(hipMemcpyAsync(c, f->d_scalar, 16, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if (c[0] == 0)
		return BTLBF_OK;
	// expected failed probes in the whole call (at most h per missing k-mer) must stay well below
	// what the fail list holds per batch
	const double miss = (double)(c[0] - c[1]) / (double)c[0];
	if (miss * live < 0.25 * (double)part_tail(scratch_budget(f)).fail_cap)
		d.route = QueryRoute::Partitioned;
	return BTLBF_OK;
}

// ---- the executors ----------------------------------------------------------------------------------------------------
// The partitioned query refines a hit bitmap, so a call that asks for counts only needs a temporary one.  Partitioned
// takes it from the runtime and synchronises before it frees it: the route also serves shards and forced modes, filters
// that may never own split scratch.  SplitCold carves it from f->split next to its other buffers, which the filter keeps
// anyway, and so needs no synchronisation.

// Partitioned: the whole buffer through the partitioned pipeline
int run_partitioned(btlbf_filter* f, const SeqArgs& a, hipStream_t s, bool* answered)
{
	DevBuf tmp_hit;
	uint8_t* hb = a.hit_bits;
	if (!hb) {
		HIP_TRY(tmp_hit.alloc(bitmap_bytes(a.len) + 16));
		hb = tmp_hit.as<uint8_t>();
	}
	SeqArgs b = a;
	b.hit_bits = nullptr;
	b.valid_bits = nullptr;
	b.counts = nullptr;
	if (int rc = part_query(f, b, hb, a.valid_bits, a.counts, s, answered, false, nullptr))
		return rc;
	if (*answered && !a.hit_bits)
		HIP_TRY(hipStreamSynchronize(s)); // tmp_hit is freed on return
	return BTLBF_OK;
}

// the direct kernel over a compacted buffer of the split query: it ADDS its clean windows and its hits to a.counts
int split_direct(btlbf_filter* f, const SeqArgs& a, int direct_op, const uint8_t* seq, uint64_t len, uint8_t* hit_bits,
                 uint8_t* valid_bits, hipStream_t s)
{
	SeqArgs d = a;
	d.seq = seq;
	d.len = len;
	d.hit_bits = hit_bits;
	d.valid_bits = valid_bits;
	ProfSpan ps(f, BTLBF_PROF_QUERY_DIRECT, s);
	REQUIRE_MATERIALIZED(f);
	HIP_TRY(launch_seq_op(direct_op, d, s));
	return BTLBF_OK;
}

// carve f->split into n buffers of sz[i] bytes (0: none); returns what they take together
uint64_t split_carve(const btlbf_filter* f, const uint64_t* sz, uint8_t** q, int n)
{
	uint64_t off = 0;
	for (int i = 0; i < n; ++i) {
		q[i] = sz[i] ? static_cast<uint8_t*>(f->split.p) + off : nullptr;
		off += sz[i];
	}
	return off;
}

// SplitCold.  Uniform reads that pass A takes through its read grid (level-0 plan `pl0`): the warm reads stay where they
// are -- pass A leaves the cold ones out by their flags (zero-staged: no entries, no bits, no counts) --, only the COLD
// reads are gathered for the direct kernel, and their answers are ORed back into the caller's bitmaps.  The first version
// gathered the warm reads as well (15 GB copied and 15 GB of HBM that the partition scratch then lacked: a third batch)
// and merged every word of the bitmaps from two sources.
int run_split_cold(btlbf_filter* f, const SeqArgs& a, int direct_op, hipStream_t s, const SplitState& st, const PartPlan& pl0,
                   bool* answered)
{
	const uint32_t L = st.L;
	const uint64_t n_cold = st.n_cold, cold_len = n_cold * L;
	const bool wv = a.valid_bits != nullptr;
	const uint64_t szm[5] = {up256(cold_len + 16), up256(bitmap_bytes(cold_len) + 16), wv ? up256(bitmap_bytes(cold_len) + 16) : 0,
	                         up256(n_cold * 4 + 16), a.hit_bits ? 0 : up256(bitmap_bytes(a.len) + 16)};
	uint64_t need = 0;
	for (uint64_t v : szm)
		need += v;
	// (a buffer left behind by a call that gathered the warm reads as well -- 19 GB for 10^8 reads -- is given back
	// first: the partition scratch is planned from the free HBM, and with that much less of it the pass would need
	// a third batch, i.e. a third sweep of the array)
	if (f->split.bytes > 4 * need + (1ull << 30))
		f->split.release();
	if (!f->split.grow(need, f->device))
		return BTLBF_OK; // no room for the gathered reads
	uint8_t* q[5];
	split_carve(f, szm, q, 5);
	uint8_t *cold_p = q[0], *cold_hit_p = q[1], *cold_valid_p = q[2];
	uint32_t* cold_index = reinterpret_cast<uint32_t*>(q[3]);
	uint8_t* hb = a.hit_bits ? a.hit_bits : q[4];
	{
		ProfSpan ps(f, BTLBF_PROF_QUERY_RESOLVE, s);
		HIP_TRY(launch_flag_prefix(st.d_flags, st.n_reads, st.d_prefix, s));
		HIP_TRY(launch_gather_cold_reads(a.seq, st.n_reads, L, st.d_flags, st.d_prefix, cold_p, cold_index, s));
		HIP_TRY(hipMemsetAsync(cold_hit_p + bitmap_bytes(cold_len), 0, 16, s)); // (the merge reads a word further)
		if (wv)
			HIP_TRY(hipMemsetAsync(cold_valid_p + bitmap_bytes(cold_len), 0, 16, s));
	}
	// part_query's two special parameters have this one user.  b.read_mask leaves the flagged reads out -- no bits, no
	// counts --, so with defer_hit_count = true counts[1] is left alone: the hits are counted below, from the bitmap the
	// cold reads' answers have been merged into.  level0 = &pl0: the plan the read grid was checked against is the one
	// that runs (part_prepare does not plan level 0 again).
	SeqArgs b = a;
	b.read_mask = reinterpret_cast<const uint32_t*>(st.d_flags);
	b.hit_bits = b.valid_bits = nullptr;
	b.counts = nullptr;
	bool done_w = false;
	if (int rc = part_query(f, b, hb, a.valid_bits, a.counts, s, &done_w, true, &pl0))
		return rc;
	if (!done_w)
		return BTLBF_OK; // no room for the partition scratch (the prefix sums and the gather stay issued)
	if (int rc = split_direct(f, a, direct_op, cold_p, cold_len, cold_hit_p, cold_valid_p, s)) // (its hits: recounted below)
		return rc;
	{
		ProfSpan ps(f, BTLBF_PROF_QUERY_RESOLVE, s);
		HIP_TRY(launch_merge_cold_bitmaps(n_cold, L, cold_index, reinterpret_cast<const uint64_t*>(cold_hit_p),
		                                  reinterpret_cast<const uint64_t*>(cold_valid_p), reinterpret_cast<uint64_t*>(hb),
		                                  reinterpret_cast<uint64_t*>(a.valid_bits), s));
		if (a.counts) { // hits = set bits of the finished bitmap
			HIP_TRY(hipMemsetAsync(a.counts + 1, 0, 8, s));
			HIP_TRY(launch_popcount(hb, bitmap_bytes(a.len), 0, 0, reinterpret_cast<unsigned long long*>(a.counts) + 1, s));
		}
	}
	*answered = true;
	return BTLBF_OK;
}

// SplitWarm.  The reads are compacted into a warm and a cold buffer, the warm one takes the partitioned path (a buffer of
// its own length, planned for itself), the cold one the early-exit gather kernel, and the two bitmaps are merged back into
// the caller's layout.
int run_split_warm(btlbf_filter* f, const SeqArgs& a, int direct_op, hipStream_t s, const SplitState& st, bool* answered)
{
	const uint32_t L = st.L;
	const uint64_t warm_len = (st.n_reads - st.n_cold) * L, cold_len = st.n_cold * L;
	const bool wv = a.valid_bits != nullptr;
	const uint64_t sz[6] = {up256(warm_len + 16), up256(cold_len + 16), up256(bitmap_bytes(warm_len) + 16),
	                        up256(bitmap_bytes(cold_len) + 16), wv ? up256(bitmap_bytes(warm_len) + 16) : 0,
	                        wv ? up256(bitmap_bytes(cold_len) + 16) : 0};
	// sized for any split of a buffer this long, so that the next call's ratio does not move memory
	const uint64_t worst = up256(a.len + 32) + 512 + (wv ? 2 : 1) * (up256(bitmap_bytes(a.len) + 32) + 512);
	if (!f->split.grow(worst, f->device))
		return BTLBF_OK; // no room for the compacted copies
	uint8_t* bufs[6];
	if (split_carve(f, sz, bufs, 6) > f->split.bytes)
		return fail(BTLBF_EINVAL, "split query: buffer arithmetic");
	uint8_t *warm_p = bufs[0], *cold_p = bufs[1], *warm_hit_p = bufs[2], *cold_hit_p = bufs[3], *warm_valid_p = bufs[4],
	        *cold_valid_p = bufs[5];
	{
		ProfSpan ps(f, BTLBF_PROF_QUERY_RESOLVE, s);
		HIP_TRY(launch_flag_prefix(st.d_flags, st.n_reads, st.d_prefix, s));
		HIP_TRY(launch_compact_reads(a.seq, st.n_reads, L, st.d_flags, st.d_prefix, warm_p, cold_p, s));
		// the merge reads one word past the last bit of a compacted bitmap
		HIP_TRY(hipMemsetAsync(warm_hit_p + bitmap_bytes(warm_len), 0, 16, s));
		HIP_TRY(hipMemsetAsync(cold_hit_p + bitmap_bytes(cold_len), 0, 16, s));
		if (a.valid_bits) {
			HIP_TRY(hipMemsetAsync(warm_valid_p + bitmap_bytes(warm_len), 0, 16, s));
			HIP_TRY(hipMemsetAsync(cold_valid_p + bitmap_bytes(cold_len), 0, 16, s));
		}
	}
	if (a.counts)
		HIP_TRY(hipMemsetAsync(a.counts, 0, 16, s));
	SeqArgs b = a;
	b.seq = warm_p;
	b.len = warm_len;
	b.hit_bits = b.valid_bits = nullptr;
	b.counts = nullptr;
	bool done_w = false;
	if (int rc = part_query(f, b, warm_hit_p, warm_valid_p, a.counts, s, &done_w, false, nullptr))
		return rc;
	int rc = BTLBF_OK;
	if (!done_w) // no room for the partition scratch: the gather kernel does the warm reads too
		rc = split_direct(f, a, direct_op, warm_p, warm_len, warm_hit_p, warm_valid_p, s);
	if (rc || (rc = split_direct(f, a, direct_op, cold_p, cold_len, cold_hit_p, cold_valid_p, s)))
		return rc;
	if (a.hit_bits || a.valid_bits) {
		ProfSpan ps(f, BTLBF_PROF_QUERY_RESOLVE, s);
		HIP_TRY(launch_merge_split_bitmaps(a.len, L, st.d_flags, st.d_prefix, reinterpret_cast<uint64_t*>(warm_hit_p),
		                                   reinterpret_cast<uint64_t*>(cold_hit_p), reinterpret_cast<uint64_t*>(warm_valid_p),
		                                   reinterpret_cast<uint64_t*>(cold_valid_p), reinterpret_cast<uint64_t*>(a.hit_bits),
		                                   reinterpret_cast<uint64_t*>(a.valid_bits), s));
	}
	*answered = true;
	return BTLBF_OK;
}

} // namespace

namespace btlbf {

int contains_routed(btlbf_filter* f, const SeqArgs& a, int op, hipStream_t s, bool* answered)
{
	*answered = false;
	QueryDecision d;
	if (int rc = decide_route(f, a, s, d))
		return rc;
	// Every executor leaves *answered false where its route cannot run, and the caller's direct kernel over the whole
	// buffer is the downgrade:
	//   Partitioned  the partition scratch does not fit (part_prepare): nothing was launched
	//   SplitCold    f->split does not grow, or the masked partitioned query finds no room: the prefix sums and the gather
	//                that were issued before it stay issued
	//   SplitWarm    f->split does not grow.  A warm partitioned query that finds no room is no downgrade of the call: the
	//                gather kernel runs over the warm buffer too, and the call is answered
	switch (d.route) {
	case QueryRoute::Direct:
		return BTLBF_OK;
	case QueryRoute::Partitioned:
		return run_partitioned(f, a, s, answered);
	case QueryRoute::SplitCold:
		return run_split_cold(f, a, op, s, d.split, d.level0, answered);
	case QueryRoute::SplitWarm:
		return run_split_warm(f, a, op, s, d.split, answered);
	}
	return BTLBF_OK;
}

} // namespace btlbf
