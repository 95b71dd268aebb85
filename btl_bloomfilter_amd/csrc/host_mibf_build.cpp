// csrc/host_mibf_build.cpp -- a multi-index Bloom filter from FASTA / FASTQ files (btlbf_mibf_build_fastx: stages 1-4),
// the window count it sizes the bit vector from (btlbf_count_windows_seqs / _fastx; mibf_build_kernels.hip) and
// calcOptimalSize.  The contracts are in include/btlbf.h.
//
// Every pass is the same loop over the files (each_batch): one sequential parser per file on a thread of its own (Side,
// fastx_side.hpp, as the classifier has it), whole records only.  A parser batch is a device batch: its bases and offsets
// go to one of two device slots on the copy stream, and while the pass's call for batch j runs on the compute stream
// batch j + 1 is taken from the parser and copied into the other slot.  The calls are the public stage calls with
// BTLBF_DEVICE (insert_seqs, mibf_insert_ids_seqs, mibf_saturate_seqs): they plan on the host and the loop synchronises
// the compute stream after each, so a slot is free again when its batch's call has returned.
#include "../../include/btlbf.h"
#include "internal.hpp"
#include "host_internal.hpp"
#include "fastx_side.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace btlbf;

extern "C" uint64_t btlbf_mibf_optimal_size(uint64_t entries, unsigned hash_num, double occupancy)
{
	// MIBloomFilter.hpp:84-88, operation for operation
	const uint64_t non64 = (uint64_t)(-double(entries) * double(hash_num) / log(1.0 - occupancy));
	return non64 + (64 - non64 % 64);
}

extern "C" int btlbf_count_windows_seqs(unsigned kmer_size, const char* seq, uint64_t len, const btlbf_layout* layout,
                                        uint64_t* out2, int mem, int device, void* stream)
{
	if (!out2 || (len && !seq))
		return btlbf_set_error(BTLBF_EINVAL, "null argument");
	if (kmer_size == 0 || kmer_size >= 1u << 31)
		return btlbf_set_error(BTLBF_EINVAL, "count windows: k must be 1..2^31-1, not %u", kmer_size);
	if (mem != BTLBF_HOST && mem != BTLBF_DEVICE)
		return btlbf_set_error(BTLBF_EINVAL, "mem must be BTLBF_HOST or BTLBF_DEVICE");
	if (layout && layout->starts && mem == BTLBF_HOST) {
		if (layout->starts[0] != 0 || layout->starts[layout->n_seqs] != len)
			return btlbf_set_error(BTLBF_EINVAL, "starts[0] must be 0 and starts[n_seqs] must equal len");
		for (uint64_t i = 0; i < layout->n_seqs; ++i)
			if (layout->starts[i + 1] < layout->starts[i])
				return btlbf_set_error(BTLBF_EINVAL, "starts must not decrease");
	}
	if (layout && !layout->starts && layout->read_len && len % layout->read_len)
		return btlbf_set_error(BTLBF_EINVAL, "len %llu is not a multiple of read_len %u", (unsigned long long)len,
		                       layout->read_len);
	if (btlbf_device_count() <= device || device < 0)
		return btlbf_set_error(BTLBF_EHIP, "no GPU %d: this library has no CPU path", device);
	DeviceGuard g(device);
	if (!g.ok)
		return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	SeqView v;
	OutBuf o;
	int rc;
	if ((rc = make_view(v, seq, len, layout, mem, s)) || (rc = o.prepare(out2, 16, mem, true, s)))
		return rc;
	HIP_TRY(launch_count_windows(v.d_seq, len, v.lay, kmer_size, o.as<unsigned long long>(), s));
	if (mem == BTLBF_DEVICE)
		return BTLBF_OK;
	if ((rc = o.finish(s)))
		return rc;
	HIP_TRY(hipStreamSynchronize(s)); // the staging buffers go back to the pool on return
	return BTLBF_OK;
}

namespace {

int file_readable(const char* path)
{
	FILE* fp = fopen(path, "rb");
	if (!fp)
		return btlbf_set_error(BTLBF_EIO, "file \"%s\" could not be read.", path);
	fclose(fp);
	return BTLBF_OK;
}

// a parser batch on the device
struct DevBatch {
	const char* d_bases = nullptr;
	const uint64_t* d_starts = nullptr;
	uint64_t nb = 0, ns = 0, longest = 0;
	unsigned file = 0;
};

// a file's parser thread ends with its scope, whichever way that is left
struct SideScope {
	Side s;
	~SideScope() { s.stop(); }
};

// the two streams and the two slots of the loop; grow only, free themselves
struct FileLoop {
	int device = 0;
	uint32_t k = 0, flags = 0;
	uint64_t cap = 0;
	hipStream_t copy_s = nullptr, comp_s = nullptr;
	DevScratch d_bases[2], d_starts[2];
	uint64_t n_batches = 0, n_bases = 0, n_records = 0; // of the last each_batch: n_records counts sequences
	uint64_t n_file_records = 0;                        // ... and this the parsers' records (btlbf_fastx_records)
	double seconds_parse = 0;

	int open()
	{
		HIP_TRY(hipStreamCreateWithFlags(&copy_s, hipStreamNonBlocking));
		HIP_TRY(hipStreamCreateWithFlags(&comp_s, hipStreamNonBlocking));
		return BTLBF_OK;
	}
	~FileLoop() // the buffers go after this: none while work is pending
	{
		for (hipStream_t s : {comp_s, copy_s})
			if (s) {
				(void)hipStreamSynchronize(s);
				(void)hipStreamDestroy(s);
			}
	}

	// the copies of a batch into slot `sl`, queued on the copy stream
	int stage(const HostBatch& b, int sl, unsigned file, DevBatch* out)
	{
		if (b.starts[0] != 0 || b.starts[b.ns] != b.nb)
			return fail(BTLBF_EINVAL, "internal error: a parser batch of %llu bytes with offsets %llu..%llu",
			            (unsigned long long)b.nb, (unsigned long long)b.starts[0], (unsigned long long)b.starts[b.ns]);
		if (!d_bases[sl].keep_room(b.nb + 64, device) || !d_starts[sl].keep_room((b.ns + 1) * 8, device))
			return fail(BTLBF_ENOMEM, "miBF build: a batch of %llu bytes", (unsigned long long)b.nb);
		if (b.nb)
			HIP_TRY(hipMemcpyAsync(d_bases[sl].p, b.bases, b.nb, hipMemcpyHostToDevice, copy_s));
		HIP_TRY(hipMemcpyAsync(d_starts[sl].p, b.starts, (b.ns + 1) * 8, hipMemcpyHostToDevice, copy_s));
		out->d_bases = d_bases[sl].as<char>();
		out->d_starts = d_starts[sl].as<uint64_t>();
		out->nb = b.nb;
		out->ns = b.ns;
		out->file = file;
		out->longest = 0;
		for (uint64_t i = 0; i < b.ns; ++i)
			out->longest = std::max(out->longest, b.starts[i + 1] - b.starts[i]);
		return BTLBF_OK;
	}

	// on_batch(const DevBatch&) for every parser batch of every file, in order; it returns with its work on comp_s done.
	// records_per_file (optional): the sequences of each file
	template <class F>
	int each_batch(const char* const* paths, unsigned n_paths, uint64_t* records_per_file, F on_batch)
	{
		n_batches = n_bases = n_records = n_file_records = 0;
		seconds_parse = 0;
		int rc;
		for (unsigned j = 0; j < n_paths; ++j) {
			SideScope sc;
			Side& side = sc.s;
			// the parser's pinned buffers need the device to be current (the caller's guard)
			if ((rc = btlbf_fastx_open(&side.r, paths[j], flags, k, cap)))
				return rc;
			side.th = std::thread([&side] { side.run(); });
			uint64_t file_records = 0;
			HostBatch cur;
			DevBatch dev[2];
			int sl = 0;
			if ((rc = side.take(&cur)) || (cur.ns && (rc = stage(cur, sl, j, &dev[sl]))))
				return rc;
			while (cur.ns) {
				// batch `cur` is on the device before its host buffers go back to the parser, which take() does
				HIP_TRY(hipStreamSynchronize(copy_s));
				HostBatch nxt;
				if ((rc = side.take(&nxt)) || (nxt.ns && (rc = stage(nxt, sl ^ 1, j, &dev[sl ^ 1]))))
					return rc;
				if ((rc = on_batch(dev[sl])))
					return rc;
				++n_batches;
				n_bases += dev[sl].nb;
				file_records += dev[sl].ns;
				cur = nxt;
				sl ^= 1;
			}
			{
				std::lock_guard<std::mutex> lk(side.mu);
				seconds_parse += side.seconds_parse;
				n_file_records += btlbf_fastx_records(side.r); // the end of input has come: the parser thread is done
			}
			n_records += file_records;
			if (records_per_file)
				records_per_file[j] = file_records;
		}
		return BTLBF_OK;
	}
};

btlbf_layout ragged(const DevBatch& b)
{
	btlbf_layout lay;
	lay.starts = b.d_starts;
	lay.n_seqs = b.ns;
	lay.read_len = 0;
	return lay;
}

// pass 0 of the builder, and count_windows_fastx: {windows, clean windows} of all files into out2
int count_pass(FileLoop& fl, const char* const* paths, unsigned n_paths, uint64_t* out2)
{
	DevScratch d_cnt;
	if (!d_cnt.grow(16, fl.device))
		return fail(BTLBF_ENOMEM, "miBF build: out of device memory");
	HIP_TRY(hipMemsetAsync(d_cnt.p, 0, 16, fl.comp_s));
	int rc = fl.each_batch(paths, n_paths, nullptr, [&](const DevBatch& b) -> int {
		HIP_TRY(launch_count_windows(reinterpret_cast<const uint8_t*>(b.d_bases), b.nb, LayoutParams{b.d_starts, b.ns, 0}, fl.k,
		                             d_cnt.as<unsigned long long>(), fl.comp_s));
		HIP_TRY(hipStreamSynchronize(fl.comp_s));
		return BTLBF_OK;
	});
	if (rc)
		return rc;
	HIP_TRY(hipMemcpyAsync(out2, d_cnt.p, 16, hipMemcpyDeviceToHost, fl.comp_s));
	HIP_TRY(hipStreamSynchronize(fl.comp_s));
	return BTLBF_OK;
}

uint64_t id_mask(unsigned id_bytes) { return 1ull << (8 * id_bytes - 1); }

// everything that can be said before the GPU is touched; *cap, *budget: batch_bytes and scratch_bytes after defaulting
int build_entry_checks(btlbf_mibf** out, btlbf_filter** stage1_out, const char* const* paths, unsigned n_paths,
                       const btlbf_mibf_build_params* p, uint64_t* cap, uint64_t* budget)
{
	if (stage1_out)
		*stage1_out = nullptr;
	if (!out)
		return btlbf_set_error(BTLBF_EINVAL, "null argument");
	*out = nullptr;
	if (!paths || !p || n_paths == 0)
		return btlbf_set_error(BTLBF_EINVAL, "miBF build: null or empty arguments");
	for (unsigned j = 0; j < n_paths; ++j)
		if (!paths[j])
			return btlbf_set_error(BTLBF_EINVAL, "miBF build: path %u is null", j);
	if (p->id_bytes != 2 && p->id_bytes != 4)
		return btlbf_set_error(BTLBF_EINVAL, "miBF: id_bytes must be 2 or 4 (uint16_t / uint32_t IDs), not %u", p->id_bytes);
	if (p->id_mode != BTLBF_MIBF_ID_PER_FILE && p->id_mode != BTLBF_MIBF_ID_PER_RECORD)
		return btlbf_set_error(BTLBF_EINVAL, "miBF build: id_mode must be BTLBF_MIBF_ID_PER_FILE or _PER_RECORD");
	if (p->saturation != BTLBF_MIBF_SAT_NONE && p->saturation != BTLBF_MIBF_SAT_SERIAL &&
	    p->saturation != BTLBF_MIBF_SAT_PARALLEL)
		return btlbf_set_error(BTLBF_EINVAL, "miBF build: saturation must be BTLBF_MIBF_SAT_NONE, _SERIAL or _PARALLEL");
	if (p->first_id == 0)
		return btlbf_set_error(BTLBF_EINVAL, "miBF build: first_id must not be 0 (0 is the empty entry)");
	const uint64_t mask = id_mask(p->id_bytes);
	if (p->id_mode == BTLBF_MIBF_ID_PER_FILE && (uint64_t)p->first_id + n_paths - 1 >= mask)
		return btlbf_set_error(BTLBF_EINVAL, "miBF build: %u files from id %u on: the last id must be below the saturation "
		                       "mask %llu of %u-byte ids", n_paths, p->first_id, (unsigned long long)mask, p->id_bytes);
	if (p->kmer_size == 0 || p->kmer_size >= 1u << 31)
		return btlbf_set_error(BTLBF_EINVAL, "miBF build: kmer_size must be at least 1");
	if (p->hash_num == 0 || p->hash_num > kMibfMaxHash)
		return btlbf_set_error(BTLBF_EINVAL, "miBF: %u hash values per window (1..%u supported)", p->hash_num, kMibfMaxHash);
	if ((p->n_seeds != 0) != (p->seeds != nullptr))
		return btlbf_set_error(BTLBF_EINVAL, "miBF build: seeds and n_seeds are given together");
	if (p->n_seeds) {
		if (p->n_seeds != p->hash_num)
			return btlbf_set_error(BTLBF_EINVAL, "miBF build: %u spaced seeds but hash_num %u (h2 = 1: one hash value per "
			                       "seed)", p->n_seeds, p->hash_num);
		for (unsigned i = 0; i < p->n_seeds; ++i)
			if (!p->seeds[i] || strlen(p->seeds[i]) != p->kmer_size)
				return btlbf_set_error(BTLBF_EINVAL, "miBF build: spaced seed %u is not of length kmer_size = %u", i,
				                       p->kmer_size);
	}
	if (p->bits == 0 && !(p->occupancy > 0.0 && p->occupancy < 1.0))
		return btlbf_set_error(BTLBF_EINVAL, "miBF build: occupancy must lie in (0, 1) to size the bit vector, not %g",
		                       p->occupancy);
	if (p->bits % 8 != 0)
		return btlbf_set_error(BTLBF_EINVAL, "ERROR: Filter Size \"%llu\" is not a multiple of 8.", (unsigned long long)p->bits);
	if (p->fastx_flags & ~(uint32_t)(BTLBF_FASTX_LINES | BTLBF_FASTX_PAGEABLE | BTLBF_FASTX_WHOLE))
		return btlbf_set_error(BTLBF_EINVAL, "miBF build: fastx_flags holds BTLBF_FASTX_LINES / _PAGEABLE only");
	*cap = p->batch_bytes ? p->batch_bytes : 64ull << 20;
	*budget = mibf_budget(p->scratch_bytes);
	if (p->saturation == BTLBF_MIBF_SAT_PARALLEL) {
		const uint64_t w = mibf_batch_windows(*cap, p->kmer_size);
		if (!mibf_parallel_fits(w, p->hash_num, *budget))
			return btlbf_set_error(BTLBF_ENOMEM, "miBF build: a batch of %llu bytes can hold %llu windows, and parallel "
			                       "saturation decides a batch at once: a scratch budget of %llu bytes would do (it is "
			                       "%llu), or a smaller batch_bytes", (unsigned long long)*cap, (unsigned long long)w,
			                       (unsigned long long)mibf_parallel_budget(w, p->hash_num), (unsigned long long)*budget);
	}
	int rc;
	for (unsigned j = 0; j < n_paths; ++j)
		if ((rc = file_readable(paths[j])))
			return rc;
	return BTLBF_OK;
}

// the passes; what they made is in *f and *m, for the caller to hand over or to destroy
int build_passes(btlbf_filter** f, btlbf_mibf** m, const char* const* paths, unsigned n_paths,
                 const btlbf_mibf_build_params* p, uint64_t cap, uint64_t budget, btlbf_mibf_build_report* rep,
                 uint64_t* records_per_file)
{
	const uint32_t h = p->hash_num;
	FileLoop fl;
	fl.device = p->device;
	fl.k = p->kmer_size;
	fl.flags = (p->fastx_flags & (BTLBF_FASTX_LINES | BTLBF_FASTX_PAGEABLE)) | BTLBF_FASTX_WHOLE;
	fl.cap = cap;
	int rc = fl.open();
	if (rc)
		return rc;
	auto close_pass = [&](int pass, double t0) {
		rep->batches[pass] = fl.n_batches;
		rep->seconds[pass] = now_s() - t0;
		rep->seconds_parse[pass] = fl.seconds_parse;
	};
	// pass 0: the entries the bit vector is sized for
	uint64_t bits = p->bits;
	if (!bits) {
		rep->entries = p->expected_entries;
		if (!rep->entries) {
			const double t0 = now_s();
			uint64_t cnt[2] = {0, 0};
			if ((rc = count_pass(fl, paths, n_paths, cnt)))
				return rc;
			rep->windows = cnt[0];
			rep->entries = rep->clean_windows = cnt[1];
			close_pass(0, t0);
		}
		bits = btlbf_mibf_optimal_size(rep->entries, h, p->occupancy);
	}
	rep->bits = bits;
	// pass 1: the stage-1 bit filter; the records and the longest of them
	if ((rc = btlbf_create(f, BTLBF_BLOOM, bits, h, p->kmer_size, 0, p->device)) ||
	    (p->n_seeds && (rc = btlbf_set_spaced_seeds(*f, p->seeds, p->n_seeds, 1))))
		return rc;
	double t0 = now_s();
	rc = fl.each_batch(paths, n_paths, records_per_file, [&](const DevBatch& b) -> int {
		rep->longest_record = std::max(rep->longest_record, b.longest);
		if (b.nb >= fl.k) {
			const btlbf_layout lay = ragged(b);
			const int e = btlbf_insert_seqs(*f, b.d_bases, b.nb, &lay, 0, BTLBF_ORDER_PARALLEL, BTLBF_DEVICE, fl.comp_s);
			if (e)
				return e;
		}
		HIP_TRY(hipStreamSynchronize(fl.comp_s));
		return BTLBF_OK;
	});
	if (rc)
		return rc;
	close_pass(1, t0);
	rep->n_records = fl.n_records;
	rep->n_bases = fl.n_bases;
	const bool per_record = p->id_mode == BTLBF_MIBF_ID_PER_RECORD;
	rep->n_ids = per_record ? rep->n_records : n_paths;
	if (per_record && rep->n_records && (uint64_t)p->first_id + rep->n_records - 1 >= id_mask(p->id_bytes))
		return fail(BTLBF_EINVAL, "miBF build: %llu records from id %u on: the last id must be below the saturation mask "
		            "%llu of %u-byte ids", (unsigned long long)rep->n_records, p->first_id,
		            (unsigned long long)id_mask(p->id_bytes), p->id_bytes);
	for (int serial = 0; serial <= (p->saturation == BTLBF_MIBF_SAT_SERIAL ? 1 : 0); ++serial)
		if (rep->longest_record > mibf_record_room(budget, h, serial))
			return fail(BTLBF_ENOMEM, "miBF build: the longest record has %llu bytes, one %s batch holds %llu under the "
			            "scratch budget of %llu bytes: a budget of %llu bytes would do",
			            (unsigned long long)rep->longest_record, serial ? "serial saturation" : "insert",
			            (unsigned long long)mibf_record_room(budget, h, serial), (unsigned long long)budget,
			            (unsigned long long)mibf_record_budget(rep->longest_record, h, serial));
	// stage 2
	if ((rc = btlbf_mibf_create(m, *f, p->id_bytes)) || (rc = btlbf_mibf_set_scratch(*m, p->scratch_bytes)))
		return rc;
	rep->pop = btlbf_mibf_size(*m);
	// passes 2 and 3: the ids of a batch are made on the device
	DevScratch d_ids, d_c4;
	if (!d_c4.grow(32, p->device))
		return fail(BTLBF_ENOMEM, "miBF build: out of device memory");
	uint64_t before = 0; // records before the batch
	auto make_ids = [&](const DevBatch& b) -> int {
		if (!d_ids.keep_room(b.ns * 4 + 16, p->device))
			return fail(BTLBF_ENOMEM, "miBF build: the ids of %llu records", (unsigned long long)b.ns);
		HIP_TRY(launch_mibf_fill_ids(d_ids.as<uint32_t>(), b.ns, per_record ? (uint32_t)(p->first_id + before) : p->first_id + b.file,
		                             per_record ? 1 : 0, fl.comp_s));
		before += b.ns;
		return BTLBF_OK;
	};
	t0 = now_s();
	rc = fl.each_batch(paths, n_paths, nullptr, [&](const DevBatch& b) -> int {
		int e = make_ids(b);
		if (e)
			return e;
		if (b.nb >= fl.k) {
			const btlbf_layout lay = ragged(b);
			if ((e = btlbf_mibf_insert_ids_seqs(*m, b.d_bases, b.nb, &lay, d_ids.as<uint32_t>(), BTLBF_DEVICE, fl.comp_s)))
				return e;
		}
		HIP_TRY(hipStreamSynchronize(fl.comp_s));
		return BTLBF_OK;
	});
	if (rc)
		return rc;
	close_pass(2, t0);
	if (p->saturation == BTLBF_MIBF_SAT_NONE)
		return BTLBF_OK;
	const int order = p->saturation == BTLBF_MIBF_SAT_SERIAL ? BTLBF_ORDER_SERIAL : BTLBF_ORDER_PARALLEL;
	before = 0;
	t0 = now_s();
	rc = fl.each_batch(paths, n_paths, nullptr, [&](const DevBatch& b) -> int {
		int e = make_ids(b);
		if (e)
			return e;
		if (b.nb >= fl.k) {
			const btlbf_layout lay = ragged(b);
			if ((e = btlbf_mibf_saturate_seqs(*m, b.d_bases, b.nb, &lay, d_ids.as<uint32_t>(), order, d_c4.as<uint64_t>(),
			                                  BTLBF_DEVICE, fl.comp_s)))
				return e;
			uint64_t c4[4];
			HIP_TRY(hipMemcpy(c4, d_c4.p, sizeof c4, hipMemcpyDeviceToHost)); // the call wrote them with a blocking copy
			for (int i = 0; i < 4; ++i)
				rep->sat_counts4[i] += c4[i];
		}
		HIP_TRY(hipStreamSynchronize(fl.comp_s));
		return BTLBF_OK;
	});
	if (rc)
		return rc;
	close_pass(3, t0);
	return BTLBF_OK;
}

} // namespace

extern "C" int btlbf_mibf_build_fastx(btlbf_mibf** out, btlbf_filter** stage1_out, const char* const* paths, unsigned n_paths,
                                      const btlbf_mibf_build_params* p, btlbf_mibf_build_report* report,
                                      uint64_t* records_per_file)
{
	uint64_t cap = 0, budget = 0;
	int rc = build_entry_checks(out, stage1_out, paths, n_paths, p, &cap, &budget);
	if (rc)
		return rc;
	if (p->device < 0 || btlbf_device_count() <= p->device)
		return btlbf_set_error(BTLBF_EHIP, "no GPU %d: this library has no CPU path", p->device);
	const double t0 = now_s();
	btlbf_mibf_build_report rep;
	memset(&rep, 0, sizeof rep);
	btlbf_filter* f = nullptr;
	btlbf_mibf* m = nullptr;
	{
		DeviceGuard g(p->device);
		if (!g.ok)
			return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", p->device);
		rc = build_passes(&f, &m, paths, n_paths, p, cap, budget, &rep, records_per_file);
	}
	rep.seconds_total = now_s() - t0;
	if (report)
		*report = rep;
	if (rc) {
		const std::string err = btlbf_last_error();
		btlbf_mibf_destroy(m);
		(void)btlbf_destroy(f);
		return btlbf_set_error(rc, "%s", err.c_str());
	}
	*out = m;
	if (stage1_out)
		*stage1_out = f;
	else
		(void)btlbf_destroy(f);
	return BTLBF_OK;
}

extern "C" int btlbf_count_windows_fastx(const char* path, unsigned kmer_size, uint32_t flags, uint64_t batch_bytes, int device,
                                         btlbf_fastx_stats* stats)
{
	if (!path || !stats)
		return btlbf_set_error(BTLBF_EINVAL, "null argument");
	memset(stats, 0, sizeof *stats);
	if (kmer_size == 0 || kmer_size >= 1u << 31)
		return btlbf_set_error(BTLBF_EINVAL, "count windows: k must be 1..2^31-1, not %u", kmer_size);
	int rc = file_readable(path);
	if (rc)
		return rc;
	if (device < 0 || btlbf_device_count() <= device)
		return btlbf_set_error(BTLBF_EHIP, "no GPU %d: this library has no CPU path", device);
	const double t0 = now_s();
	DeviceGuard g(device);
	if (!g.ok)
		return fail(BTLBF_EHIP, "no GPU %d: this library has no CPU path", device);
	FileLoop fl;
	fl.device = device;
	fl.k = kmer_size;
	fl.flags = flags & (BTLBF_FASTX_LINES | BTLBF_FASTX_PAGEABLE | BTLBF_FASTX_WHOLE);
	fl.cap = batch_bytes ? batch_bytes : 64ull << 20;
	uint64_t cnt[2] = {0, 0};
	if ((rc = fl.open()) || (rc = count_pass(fl, &path, 1, cnt)))
		return rc;
	stats->n_records = fl.n_file_records;
	stats->n_bases = fl.n_bases;
	stats->n_windows = cnt[1];
	stats->n_hits = cnt[0];
	stats->n_batches = fl.n_batches;
	stats->seconds_parse = fl.seconds_parse;
	stats->seconds_total = now_s() - t0;
	return BTLBF_OK;
}
